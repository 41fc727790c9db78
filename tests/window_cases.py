"""Inputs of the window-model fixture (tests/golden/window_model.npz), regenerated from seeds on both sides: the tool that
runs the reference (tools/make_goldens_window.py) and the tests; only the reference's outputs are stored."""
import numpy as np
import torch

NB_CLS = 80
TINY_WIDTHS = (256, 800)          # 64 x 256 -> N = 64; 64 x 800 -> N = 200 (ragged for windows of 16 and 64-token tiles)
MASK_SEED, MASK_RATIO, MAX_SPAN = 5, 0.4, 8
FULL_GRAD = 4096                  # gradients up to this size are stored whole, larger ones as a fixed sample


def sample_index(n, k=1024):
    return np.random.default_rng(n).choice(n, size=k, replace=False)


def perturb(m):
    """seeded values for what the constructor leaves constant: relative-position tables, LayerNorm affines, BatchNorm
    affines and running statistics (the same draws on the reference and on the drop-in)"""
    r = np.random.default_rng(77)
    with torch.no_grad():
        for n, t in m.state_dict(keep_vars=True).items():
            if n.endswith("relative_position_bias_table"):
                t.copy_(torch.from_numpy(r.standard_normal(tuple(t.shape)) * 0.5))
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


def tiny_batch(W, B=2):
    r = np.random.default_rng(300 + W)
    x = torch.from_numpy(r.random((B, 1, 64, W)).astype(np.float32))
    lengths = torch.tensor([7, 12], dtype=torch.int32)[:B]
    targets = torch.from_numpy(r.integers(1, NB_CLS, size=int(lengths.sum())).astype(np.int32))
    return x, targets, lengths


def d768_images(B=2):
    r = np.random.default_rng(768)
    return torch.from_numpy(r.random((B, 1, 64, 512)).astype(np.float32))
