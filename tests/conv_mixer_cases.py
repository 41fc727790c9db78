"""Shared by tools/make_goldens_conv_mixer.py and the conv-mixer tests: the cases of tests/golden/conv_mixer.npz and the
seeded perturbation that turns a freshly initialised ConvLocalMixer1D into the fixture's module (a fresh BatchNorm has
weight 1, bias 0 and unit running statistics, which would hide mistakes in all four)."""
import torch

D, K, INIT_SEED = 64, 7, 123
# name -> (B, N, use_bn, seed of the inputs)
CASES = {"b3n33": (3, 33, True, 1), "b2n5": (2, 5, True, 2), "nobn": (2, 5, False, 3)}


def perturb(module, seed=5):
    """in place, float32, on the CPU: every parameter += 0.1 * randn, running_mean = 0.3 * randn, running_var in [0.5, 1.5)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(module.named_parameters()):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        for n, b in sorted(module.named_buffers()):
            if n.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return module


def inputs(case):
    """(x, dy) float32 [B, N, D]"""
    B, N, _, seed = CASES[case]
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
