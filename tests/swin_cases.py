"""Shared by tools/make_goldens_swin.py and the Swin tests: the modules and cases of tests/golden/swin.npz, the seeded
perturbation that turns freshly initialised modules into the fixture's (a fresh LayerNorm has weight 1 and bias 0 and the
table sits at 0.02-sized values, which would hide mistakes in all three), the probes that stand in for the large gradients,
and the shapes and seeded inputs of the kernel tests.

The fixture has to stay below 1 MB, and the blocks of the chain alone hold two million parameters.  So:
  * sd.* is stored for the four small modules of INIT only; a module of a case is rebuilt from its seed (build below) and
    the fixture keeps the float64 sum of every entry of its state_dict, which the tests compare first;
  * a gradient of more than PROBE_ABOVE elements (a weight matrix G [out, in]) is stored as its two products with seeded
    probe vectors, G v and u G, plus its largest magnitude: any wrong element of G moves both.  That serves the float64
    comparison of tests/swin_refs.py with the fork (1e-10, where a probe is as sharp as the elements).  The GPU tests do not
    judge through probes: they compare every gradient element with swin_refs over the same state_dict."""
import torch

INIT_SEED = 123
PROBE_ABOVE = 1024
# per element, what a rebuilt parameter may differ by from the one the fixture was made with: nothing on the processor that
# made it; elsewhere torch's vectorised CPU code for erfinv (trunc_normal_) and the normal sampler may round the last bit of a
# float32 of magnitude 0.1 ... 1 the other way (6e-8).  A wrong seed or a missing perturbation is 0.1 per element.
SUM_TOL = 1e-6
# the four modules of init.* / sd.*: kind, constructor arguments
INIT = {"attn": ("attn", (32, 1, (4, 8)), {}),
        "block": ("block", (64, 2, (4, 8), (2, 4)), {"mlp_ratio": 2.0}),
        "merge": ("merge", (32, 64), {}),
        "comb": ("comb", (64, 64), {"drop": 0.0})}
# module cases: name -> (B, H, W, seed of the inputs, [(tag, kind, args, kwargs), ...] applied in turn)
CASES = {
    # two window rows, both shifts, four regions
    "block": (2, 8, 16, 1, [("b", "block", (64, 2, (4, 8), (2, 4)), {"mlp_ratio": 2.0})]),
    # every module and every head width: 32, 64, 128 over two heads, the fork's three windows on its three map heights
    "chain": (2, 4, 16, 2, [("b0", "block", (64, 2, (4, 8), (0, 0)), {"mlp_ratio": 2.0}),
                            ("m0", "merge", (64, 128), {}),
                            ("b1", "block", (128, 2, (2, 8), (1, 4)), {"mlp_ratio": 2.0}),
                            ("m1", "merge", (128, 256), {}),
                            ("b2", "block", (256, 2, (1, 8), (0, 0)), {"mlp_ratio": 2.0}),
                            ("b3", "block", (256, 2, (1, 8), (0, 4)), {"mlp_ratio": 2.0}),
                            ("c", "comb", (256, 256), {"drop": 0.0})]),
}

# kernel cases (B, H, W, heads, hd, wh, ww, sh, sw): one window, one head; wrap along W, two regions in the last window;
# H == wh (the roll stays inside one window row), four regions, an odd window count; two window rows, both shifts; a
# 15-token window, nothing a power of two; the fork's head count, five windows across; the fork's own map, past one
# workgroup; 1152 two-by-two windows: more (image, window) items than the 256 partial rows of the table gradient times the
# waves of a workgroup, so every wave walks more than one item
KERNEL_SHAPES = [(1, 1, 8, 1, 32, 1, 8, 0, 0), (2, 1, 16, 2, 128, 1, 8, 0, 4), (2, 2, 24, 3, 64, 2, 8, 1, 4),
                 (2, 8, 16, 2, 32, 4, 8, 2, 4), (2, 3, 10, 1, 64, 3, 5, 1, 2), (3, 4, 40, 6, 32, 4, 8, 0, 0),
                 (2, 4, 128, 6, 32, 4, 8, 2, 4), (3, 16, 96, 1, 32, 2, 2, 1, 1)]
FORK_SHAPE = (2, 4, 128, 6, 32, 4, 8, 2, 4)


def build(mods, kind, args, kwargs, **extra):
    """a module of `mods` (the fork's HTR_VT module or htrvt_amd.swin) by kind"""
    ctor = {"attn": mods.WindowAttention2D, "block": mods.SwinBlock2D, "merge": mods.HeightOnlyPatchMerging,
            "comb": mods.Combining}[kind]
    return ctor(*args, **kwargs, **extra)


def perturb(module, seed=5):
    """in place, float32, on the CPU: every parameter += 0.1 * randn"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(module.named_parameters()):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    return module


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
            H, C = H // 2, args[1]
        elif kind == "comb":
            H, C = 1, args[1]
    return B, H * W, C


def inputs(case):
    """(x [B, H*W, C], dy of the output's shape) float32"""
    B, H, W, seed, stages = CASES[case]
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randn(B, H * W, stages[0][2][0], generator=g), torch.randn(*out_shape(case), generator=g)


def probes(shape):
    """(u [out], v [in]) float64 for a gradient [out, in, ...] flattened to [out, rest]"""
    g = torch.Generator().manual_seed(shape[0] * 31 + 7)
    rest = 1
    for s in shape[1:]:
        rest *= s
    return torch.randn(shape[0], generator=g, dtype=torch.float64), torch.randn(rest, generator=g, dtype=torch.float64)


def probe(grad):
    """what the fixture keeps of a large gradient: {"gv": G v, "ug": u G, "max": max |G|}, float64"""
    G = grad.detach().double().reshape(grad.shape[0], -1)
    u, v = probes(tuple(grad.shape))
    return {"gv": G @ v, "ug": u @ G, "max": G.abs().max()}


def kernel_inputs(shape, dtype, seed=0):
    """qkv [B*H*W, 3*heads*hd] and dout [B*H*W, heads*hd] already rounded to dtype, table float32 [(2wh-1)(2ww-1), heads]
    with entries of order 1 (the parameter after training, not its 0.02 init); images and windows differ from each other"""
    B, H, W, heads, hd, wh, ww, sh, sw = shape
    g = torch.Generator().manual_seed(17 * H + 5 * W + 3 * heads + hd + wh + ww + sh + sw + seed)
    qkv = torch.randn(B * H * W, 3 * heads * hd, generator=g).to(dtype)
    dout = torch.randn(B * H * W, heads * hd, generator=g).to(dtype)
    table = torch.randn((2 * wh - 1) * (2 * ww - 1), heads, generator=g)
    return qkv, table, dout
