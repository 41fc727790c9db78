"""Shared by tools/make_goldens_svtr.py and the SVTR tests: the modules and cases of tests/golden/svtr.npz and the shapes and
seeded inputs of the kernel tests.  The devices that keep the fixture below 1 MB are swin_cases': modules rebuilt from seeds and
perturbed (a fresh LayerNorm has weight 1 and bias 0, which would hide mistakes in both), the float64 sum of every
state_dict entry to recognise a rebuilt module, and probe products for gradients of more than PROBE_ABOVE elements."""
import torch

from swin_cases import INIT_SEED, PROBE_ABOVE, SUM_TOL, perturb, probe, probes  # noqa: F401

# the four modules of init.* / sd.*: kind, constructor arguments
INIT = {"attn": ("attn", (32, 1, True, (3, 5)), {}),
        "block": ("block", (32, 1, True), {}),
        "merge": ("merge", (16, 32), {}),
        "comb": ("comb", (32, 32), {"drop": 0.0})}
# module cases: name -> (B, H, W, seed of the inputs, [(tag, kind, args, kwargs), ...] applied in turn)
CASES = {
    # a local block: H < kh, so every row sees every row, and W past one 16-column tile
    "local": (1, 6, 20, 1, [("b", "block", (64, 2, True), {})]),
    # a global block of 64 tokens: the fused kernel in bfloat16, the unfused route in float32
    "global": (1, 4, 16, 2, [("b", "block", (64, 2, False), {})]),
    # a global block of 16 tokens and one head of 64: the unfused route in both dtypes
    "global_small": (1, 2, 8, 3, [("b", "block", (64, 1, False), {})]),
    "merge_even": (2, 4, 16, 4, [("m", "merge", (16, 32), {})]),
    "merge_odd": (2, 3, 16, 5, [("m", "merge", (16, 32), {})]),
    # an odd height whose row parity classes both hold more than 128 pixels: the per-class input gradient in bfloat16
    "merge_class": (2, 7, 24, 6, [("m", "merge", (16, 32), {})]),
    "comb": (1, 4, 16, 7, [("c", "comb", (64, 64), {"drop": 0.0})]),
    # local block -> merging (8 -> 4 rows) -> global block of 48 tokens, four heads -> combining
    "chain": (1, 8, 12, 8, [("b0", "block", (64, 2, True), {}),
                            ("m0", "merge", (64, 128), {}),
                            ("b1", "block", (128, 4, False), {}),
                            ("c", "comb", (128, 128), {"drop": 0.0})]),
}

# kernel cases (B, H, W, heads, hd, kh, kw): one token; H < kh, every row sees every row; the fork's first map height, rows
# with 24 keys at the corners and all 77 in the interior; nothing a multiple of a tile; the other head width, a small box;
# boxes of one row / one column, W < kw; more images than workgroups of any one image; the fork's own map, past one workgroup
KERNEL_SHAPES = [(1, 1, 1, 1, 32, 7, 11), (2, 4, 12, 2, 32, 7, 11), (1, 16, 24, 2, 32, 7, 11), (2, 9, 37, 3, 32, 7, 11),
                 (2, 8, 40, 1, 64, 3, 5), (1, 3, 70, 2, 32, 1, 11), (1, 20, 3, 1, 32, 7, 1), (300, 2, 3, 1, 32, 7, 11),
                 (3, 16, 128, 2, 32, 7, 11)]
FORK_SHAPE = (3, 16, 128, 2, 32, 7, 11)


def build(mods, kind, args, kwargs, **extra):
    """a module of `mods` (the fork's svtr module or htrvt_amd.svtr) by kind"""
    ctor = {"attn": mods.MultiHeadSelfAttention, "block": mods.MixingBlock, "merge": mods.Merging,
            "comb": mods.Combining}[kind]
    return ctor(*args, **kwargs, **extra)


def case_modules(mods, case, **extra):
    """[(tag, kind, args, module)] of a case: each module seeded INIT_SEED + its position, then perturbed"""
    out = []
    for i, (tag, kind, args, kwargs) in enumerate(CASES[case][4]):
        torch.manual_seed(INIT_SEED + i)
        out.append((tag, kind, args, perturb(build(mods, kind, args, kwargs, **extra), seed=5 + i)))
    return out


def out_shape(case):
    """(B, tokens, channels) of the case's output"""
    B, H, W, _, stages = CASES[case]
    C = stages[0][2][0]
    for _, kind, args, _ in stages:
        if kind == "merge":
            H, C = (H - 1) // 2 + 1, args[1]
        elif kind == "comb":
            H, C = 1, args[1]
    return B, H * W, C


def inputs(case):
    """(x [B, H*W, C], dy of the output's shape) float32"""
    B, H, W, seed, stages = CASES[case]
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.randn(B, H * W, stages[0][2][0], generator=g), torch.randn(*out_shape(case), generator=g)


def kernel_inputs(shape, dtype, seed=0):
    """qkv [B*H*W, 3*heads*hd] and dout [B*H*W, heads*hd], already rounded to dtype; images and heads differ from each other"""
    B, H, W, heads, hd, kh, kw = shape
    g = torch.Generator().manual_seed(17 * H + 5 * W + 3 * heads + hd + kh + kw + seed)
    qkv = torch.randn(B * H * W, 3 * heads * hd, generator=g).to(dtype)
    dout = torch.randn(B * H * W, heads * hd, generator=g).to(dtype)
    return qkv, dout
