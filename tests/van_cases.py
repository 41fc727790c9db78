"""Shared by tools/make_goldens_van.py and the VAN tests: the cases of tests/golden/van.npz, the seeded perturbation that
turns freshly initialised modules into the fixture's (a fresh BatchNorm has weight 1, bias 0 and unit running statistics,
which would hide mistakes in all four), and the shapes and seeded inputs of the kernel tests."""
import torch

D, DEPTH, K, INIT_SEED = 32, 2, 9, 123
# module cases: name -> (B, H, W, seed of the inputs).  The reducer takes x (B, D, H, W); the mixer its output's shape (B, D, 1, W)
CASES = {"b2h4w9": (2, 4, 9, 1), "b3h3w33": (3, 3, 33, 2)}

# depthwise kernel cases (B, H, W, C, kh, kw, dil): an image smaller than the kernel; W below the dilated reach, most
# kernel rows dead; rows 9 and 10 see all seven kernel rows; an odd width and three channel octets; the mixer form past one
# tile of width; the forks' own map, past one channel block
DW_SHAPES = [(1, 1, 2, 8, 5, 5, 1), (2, 4, 7, 8, 7, 7, 3), (2, 20, 21, 8, 7, 7, 3), (2, 4, 33, 24, 5, 5, 1),
             (3, 1, 130, 64, 1, 9, 1), (2, 4, 128, 768, 7, 7, 3)]
# shapes (B, H, W, C) of the element-wise and pool kernels: one vector, an odd pixel count over three octets, past one
# workgroup of rows, past one channel block
EW_SHAPES = [(1, 1, 2, 8), (2, 3, 7, 24), (3, 4, 50, 64), (2, 2, 9, 768)]


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
    """(x (B, D, H, W), dy (B, D, 1, W)) float32 for the reducer; the mixer takes (xm, dym), both (B, D, 1, W)"""
    B, H, W, seed = CASES[case]
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.randn(B, D, H, W, generator=g), torch.randn(B, D, 1, W, generator=g),
            torch.randn(B, D, 1, W, generator=g), torch.randn(B, D, 1, W, generator=g))


def dw_inputs(shape, dtype, seed=0):
    """x, dy [B, H, W, C] already rounded to dtype; w float32 [C, kh * kw]; images differ from each other"""
    B, H, W, C, kh, kw, dil = shape
    g = torch.Generator().manual_seed(7 * H + 3 * W + C + kh + kw + dil + seed)
    x = torch.randn(B, H, W, C, generator=g).to(dtype)
    dy = torch.randn(B, H, W, C, generator=g).to(dtype)
    w = torch.randn(C, kh * kw, generator=g) * 0.4
    return x, dy, w


def ew_inputs(shape, dtype, seed=0):
    """four tensors [B, H, W, C] rounded to dtype, and scale, shift float32 [C]"""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(11 * H + W + C + seed)
    t = [torch.randn(B, H, W, C, generator=g).to(dtype) for _ in range(4)]
    return t, torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.3
