"""Inputs of the LGP-model fixture (tests/golden/lgp_model.npz), regenerated from seeds on both sides: the tool that runs
the reference (tools/make_goldens_lgp.py) and the tests; only the reference's outputs are stored."""
import numpy as np
import torch

NB_CLS = 80
TINY_WIDTHS = (256, 800)          # 64 x 256 -> N = 64 (pad 8 for windows of 12, G = N); 64 x 800 -> N = 200 (pad 4, 64 uneven bins)
MASK_SEED, MASK_RATIO, MAX_SPAN = 5, 0.4, 8
FULL_GRAD = 4096                  # gradients up to this size are stored whole, larger ones as a fixed sample


def sample_index(n, k=1024):
    return np.random.default_rng(n).choice(n, size=k, replace=False)


def perturb(m):
    """seeded values for what the constructor leaves constant (the same draws on the reference and on the drop-in): a
    different logit_alpha per block, LayerNorm affines, every Linear bias (zero after init: a zero qkv bias would make the
    padding keys of a ragged window trivial), BatchNorm affines and running statistics"""
    r = np.random.default_rng(91)
    with torch.no_grad():
        for n, t in m.state_dict(keep_vars=True).items():
            if n.endswith("logit_alpha"):
                t.copy_(torch.tensor(r.uniform(-1.5, 1.5)))
            elif (".norm" in n or n.startswith("norm.")) and (n.endswith(".weight") or n.endswith(".bias")):
                base = 1.0 if n.endswith(".weight") else 0.0
                t.copy_(torch.from_numpy(base + 0.1 * r.standard_normal(tuple(t.shape))))
            elif "bn" in n or "downsample.1" in n:
                if n.endswith("running_var"):
                    t.copy_(torch.from_numpy(0.5 + r.random(tuple(t.shape))))
                elif n.endswith("running_mean") or n.endswith(".bias"):
                    t.copy_(torch.from_numpy(0.1 * r.standard_normal(tuple(t.shape))))
                elif n.endswith(".weight"):
                    t.copy_(torch.from_numpy(1.0 + 0.1 * r.standard_normal(tuple(t.shape))))
            elif n.endswith(".bias") and t.dim() == 1:          # qkv / proj / fuse / fc1 / fc2 / head
                t.copy_(torch.from_numpy(0.2 * r.standard_normal(tuple(t.shape))))


def tiny_batch(W, B=2):
    r = np.random.default_rng(500 + W)
    x = torch.from_numpy(r.random((B, 1, 64, W)).astype(np.float32))
    lengths = torch.tensor([7, 12], dtype=torch.int32)[:B]
    targets = torch.from_numpy(r.integers(1, NB_CLS, size=int(lengths.sum())).astype(np.int32))
    return x, targets, lengths


def d768_images(B=1):
    r = np.random.default_rng(769)
    return torch.from_numpy(r.random((B, 1, 64, 512)).astype(np.float32))
