"""Shared by tools/make_goldens_squeezeformer.py and the Conformer / SqueezeFormer tests: the modules and cases of
tests/golden/squeezeformer.npz, the seeded perturbation that turns freshly initialised modules into the fixture's (a fresh
LayerNorm / GroupNorm has weight 1 and bias 0, which would hide mistakes in both), the probes that stand in for the large
tensors, and the shapes and seeded inputs of the kernel tests.

The fixture has to stay below 1 MB, and one block at dim 256 alone holds 0.9 million parameters.  So, as swin_cases does:
  * a module of a case is rebuilt from its seed (build / case_module below) and the fixture keeps the float64 sum of every
    entry of its state_dict, which the tests compare first;
  * a tensor of more than PROBE_ABOVE elements (an output, a gradient) is stored as its product G v with a seeded probe
    vector: any wrong element moves it.  That serves the float64 comparison of
    tests/squeezeformer_refs.py with the fork (1e-10, where a probe is as sharp as the elements).  The GPU tests do not
    judge through probes: they compare every element with squeezeformer_refs over the same state_dict."""
from functools import partial

import torch
import torch.nn as nn

INIT_SEED = 123
PROBE_ABOVE = 64
SUM_TOL = 1e-6          # per element, what a rebuilt parameter may differ by on another processor (see swin_cases)
NORM_EPS = 1e-6         # the forks' norm_layer = partial(nn.LayerNorm, eps=1e-6)
OFF = dict(ff_dropout=0.0, attn_dropout=0.0, conv_dropout=0.0)

# the modules of init.*: kind, constructor arguments (the fork's defaults, dropout rates included)
INIT = {"ffn": ("ffn", (32, 64), {}),
        "conv": ("conv", (32,), {"kernel_size": 7}),
        "se": ("se", (32,), {}),
        "cblock": ("cblock", (64, 2, 16), {"mlp_ratio": 2.0}),
        "sblock": ("sblock", (64, 2, 16), {"mlp_ratio": 2.0}),
        "encoder": ("encoder", (64, 2, 16, 3), {"mlp_ratio": 2.0, "drop_path_total": 0.0})}


def _block(kind, dim, heads, N):
    return (kind, (dim, heads, N), dict(mlp_ratio=2.0, **OFF), 2, N)


# module cases: name -> (kind, args, kwargs, B, N); every rate is zero, so train and eval mode compute the same
CASES = {
    "ffn": ("ffn", (32, 64), {"dropout": 0.0}, 2, 5),
    "conv_k3": ("conv", (48,), {"kernel_size": 3, "dropout": 0.0}, 3, 33),
    "conv_k7": ("conv", (16,), {"kernel_size": 7, "dropout": 0.0}, 2, 5),
    "conv_wide": ("conv", (64,), {"kernel_size": 15, "dropout": 0.0, "expansion": 2.0}, 2, 16),
    "se_clamp": ("se", (8,), {}, 1, 1),
    "se_24": ("se", (24,), {}, 3, 33),
    "down_5": ("down", (), {}, 3, 5),
    "down_33": ("down", (), {}, 3, 33),
    "up_5": ("up", (), {}, 3, 2),
    "up_33": ("up", (), {}, 3, 16),
}
for _k in ("cblock", "sblock"):
    for _d in (128, 256):
        for _n in (16, 33):
            CASES[f"{_k}_d{_d}_n{_n}"] = _block(_k, _d, 2, _n)
for _depth in (2, 3):
    for _n in (16, 33):
        CASES[f"enc_l{_depth}_n{_n}"] = ("encoder", (128, 2, _n, _depth), dict(mlp_ratio=2.0, drop_path_total=0.0, **OFF), 2, _n)
RESAMPLE_DIM = 8
UP_TARGET = {"up_5": 5, "up_33": 33}
DROPOUT_CASE = ("conv", (64,), {"kernel_size": 3, "dropout": 0.1}, 3, 33)

# kernel shapes (B, N, C, k) of the GroupNorm mixer: one token, no taps; an image shorter than a run; runs and workgroups
# straddling image boundaries, a ragged last run, channel vectors not filling a workgroup; the widest window; more images than
# runs per workgroup; the forks' two stages
MIXER_SHAPES = [(1, 1, 8, 1), (2, 5, 8, 3), (3, 33, 24, 7), (2, 16, 64, 15), (5, 7, 40, 3), (2, 128, 384, 3), (2, 64, 384, 3)]
SE_SHAPES = [(1, 1, 8), (3, 33, 24), (2, 128, 768)]
RESAMPLE_N0 = (2, 5, 33, 128)
RESAMPLE_D = (8, 24)
RESAMPLE_B = 3


def se_hidden(D, ratio=0.25):
    return max(8, int(D * ratio))


def build(mods, kind, args, kwargs, **extra):
    """a module of `mods` (the fork's HTR_VT module or htrvt_amd.conformer) by kind"""
    ctor = {"ffn": mods.FeedForward, "conv": mods.ConvModule, "se": mods.SqueezeExcite1D, "down": mods.Downsample1D,
            "up": mods.Upsample1D, "cblock": mods.ConformerBlock, "sblock": mods.SqueezeConformerBlock,
            "encoder": mods.SqueezeFormerEncoder}[kind]
    kwargs = dict(kwargs)
    if kind in ("cblock", "sblock", "encoder"):
        kwargs["norm_layer"] = partial(nn.LayerNorm, eps=NORM_EPS)
    return ctor(*args, **kwargs, **extra)


def perturb(module, seed=5):
    """in place, float32, on the CPU: every parameter += 0.1 * randn"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(module.named_parameters()):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    return module


def case_module(mods, case, **extra):
    """the case's module: seeded INIT_SEED, then perturbed"""
    kind, args, kwargs = (CASES[case] if isinstance(case, str) else case)[:3]
    torch.manual_seed(INIT_SEED)
    return perturb(build(mods, kind, args, kwargs, **extra))


def case_dim(case):
    kind, args = CASES[case][:2]
    return RESAMPLE_DIM if kind in ("down", "up") else args[0]


def out_tokens(case):
    kind, _, _, _, N = CASES[case]
    return N // 2 if kind == "down" else UP_TARGET[case] if kind == "up" else N


def inputs(case, spec=None):
    """(x [B, N, dim], dy of the output's shape) float32; image b is scaled by 1 + b / 2 and shifted by b / 4"""
    if spec is None:
        _, _, _, B, N = CASES[case]
        D, No, seed = case_dim(case), out_tokens(case), sorted(CASES).index(case)
    else:
        (_, args, _, B, N), seed = spec, 99
        D, No = args[0], N
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randn(B, N, D, generator=g)
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    return x * (1 + 0.5 * b) + 0.25 * b, torch.randn(B, No, D, generator=g)


def probe(t, activation=False):
    """what the fixture keeps of a large tensor: G v, float64, with G the tensor as a matrix -- an activation [B, N, D] as
    its rows [B*N, D], a weight [out, in, ...] as [out, rest], a vector as one row -- and v a seeded probe vector.  Any
    wrong element moves the product of its row."""
    t = t.detach().double()
    G = t.reshape(-1, t.shape[-1]) if activation else t.reshape(1, -1) if t.dim() == 1 else t.reshape(t.shape[0], -1)
    g = torch.Generator().manual_seed(G.shape[1] * 31 + 7)
    return G @ torch.randn(G.shape[1], generator=g, dtype=torch.float64)


def mixer_inputs(B, N, C, k, dtype, seed=0):
    """u [B*N, 2C], ds [B*N, C] already rounded to dtype, and the float32 parameters.  Image b is scaled by 1 + b and
    shifted by b, so batch-wide or a neighbour's statistics miss every gate; the depthwise bias is of order 1"""
    g = torch.Generator().manual_seed(31 * N + C + k + seed)
    u = torch.randn(B, N, 2 * C, generator=g) * 1.5
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    u[:, :, :C] = u[:, :, :C] * (1 + b) + b
    u = u.view(B * N, 2 * C).to(dtype)
    ds = torch.randn(B * N, C, generator=g).to(dtype)
    w = torch.randn(C, k, generator=g) * 0.4
    bias = torch.randn(C, generator=g) + 0.5
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.3
    return u, ds, w, bias, gamma, beta


def se_inputs(B, N, D, dtype, seed=0):
    g = torch.Generator().manual_seed(7 * N + D + seed)
    H = se_hidden(D)
    x = torch.randn(B, N, D, generator=g)
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    x = (x * (1 + b) + 0.5 * b).view(B * N, D).to(dtype)
    dy = torch.randn(B * N, D, generator=g).to(dtype)
    w1, b1 = torch.randn(H, D, generator=g) * D ** -0.5, torch.randn(H, generator=g) * 0.3
    w2, b2 = torch.randn(D, H, generator=g) * H ** -0.5, torch.randn(D, generator=g) * 0.3
    return x, dy, w1, b1, w2, b2
