"""Train-mode restatements for the convolutional forks' regularisers, no GPU needed:

  * the five modules of htrvt_amd.conformer that take rates (FeedForward, ConvModule, ConformerBlock,
    SqueezeConformerBlock, SqueezeFormerEncoder) with EXPLICIT masks, on the pieces of tests/squeezeformer_refs.py and in
    the dtype of their inputs (float64 is the yardstick); gradients by autograd.  tests/test_conformer_dropout_cpu.py ties
    them to the forks' own modules through tests/golden/conformer_dropout.npz;
  * the masks from seeds: the keys of htrvt_residual_dropout / csrc/dropnorm.hip and of the attention `drop=`, over
    attn_dropout_refs.keep_elems (the numpy restatement of csrc/dropout_common.h);
  * the two kernels of csrc/dropnorm.hip, written from include/htrvt.h;
  * the cases of the fixture, shared by tools/make_goldens_conformer_dropout.py and the tests.

A block's masks are a dict: "E" [4][B*N, D] and "S" [4][B], the element and sample keeps (1 / 0, floating) of the sites
ffn1, attn, conv, ffn2, and "A" [B, heads, N, N], the keep of the attention probabilities.  Its rates are a dict: "E" the
four element rates, "S" the drop-path rate, "A" the attention rate.  An encoder takes a list of each, stage1 then stage2."""
import numpy as np
import torch

import attn_dropout_refs as A
import kernel_refs as R
import squeezeformer_cases as C
import squeezeformer_refs as S

SITES = ("ffn1", "attn", "conv", "ffn2")
FF, ATT, CONV, PATH = 0.1, 0.1, 0.1, 0.4
_RATES = dict(ff_dropout=FF, attn_dropout=ATT, conv_dropout=CONV)
B, N, D, HEADS = 5, 40, 64, 2
# name -> (kind, args, kwargs, B, N) as squeezeformer_cases.CASES.  The encoder runs at 64 tokens: its second stage then has
# 32, where bfloat16 still takes the fused attention (below that, 20 tokens are off the 16-byte row and the padded route
# refuses attention dropout); its two blocks get the drop-path rates linspace(0, 0.4, 2) = 0 and 0.4
CASES = {
    "ffn": ("ffn", (D, 2 * D), {"dropout": FF}, B, N),
    "conv": ("conv", (D,), {"kernel_size": 3, "dropout": CONV, "drop_path": PATH}, B, N),
    "cblock": ("cblock", (D, HEADS, N), dict(mlp_ratio=2.0, drop_path=PATH, **_RATES), B, N),
    "sblock": ("sblock", (D, HEADS, N), dict(mlp_ratio=2.0, drop_path=PATH, **_RATES), B, N),
    "encoder": ("encoder", (D, HEADS, 64, 2), dict(mlp_ratio=2.0, drop_path_total=PATH, **_RATES), B, 64),
}


def case_module(mods, case, **extra):
    return C.case_module(mods, CASES[case], **extra)


def inputs(case):
    return C.inputs(None, CASES[case])


def block_rates(case):
    """the rates dict of a case's block(s): one dict, or for the encoder a list (stage1 then stage2)"""
    kind, args, kw = CASES[case][:3]
    if kind == "encoder":
        return [dict(E=(FF, FF, CONV, FF), S=float(p), A=ATT) for p in torch.linspace(0, kw["drop_path_total"], args[3])]
    return dict(E=(FF, FF, CONV, FF), S=PATH, A=ATT)


# ------------------------------------------------------------------ masks from seeds
def site_masks(seeds, rows, Dm, rows_per_sample, p, p_path):
    """(keepE bool [rows, Dm], keepS bool [samples]) of a residual site: element key (seeds[0], row * Dm + col), sample key
    (seeds[1], row // rows_per_sample); a rate of 0 keeps everything"""
    nb = (rows + rows_per_sample - 1) // rows_per_sample
    e = A.keep_elems(seeds[0], np.arange(rows * Dm, dtype=np.uint64), p).reshape(rows, Dm) if p > 0 else np.ones((rows, Dm), bool)
    s = A.keep_elems(seeds[1], np.arange(nb, dtype=np.uint64), p_path) if p_path > 0 else np.ones(nb, bool)
    return e, s


def site_factor(seeds, rows, Dm, rows_per_sample, p, p_path):
    """float64 [rows, Dm]: keepE / (1 - p) * keepS / (1 - p_path)"""
    e, s = site_masks(seeds, rows, Dm, rows_per_sample, p, p_path)
    f = torch.from_numpy(e).double() * torch.from_numpy(s).double().repeat_interleave(rows_per_sample)[:rows, None]
    return f / (1.0 - p) / (1.0 - p_path)


def block_masks(seeds, rates, Bm, Nm, Dm, heads):
    """the masks dict of a block from its nine seeds (htrvt_amd.conformer.ConformerBlock.last_drop_seeds)"""
    seeds = [int(v) for v in seeds]
    E, Sm = [], []
    for i, p in enumerate(rates["E"]):
        e, s = site_masks(seeds[2 * i:2 * i + 2], Bm * Nm, Dm, Nm, p, rates["S"])
        E.append(torch.from_numpy(e).double())
        Sm.append(torch.from_numpy(s).double())
    a = A.keep_mask(seeds[8], Bm, heads, Nm, rates["A"]) if rates["A"] > 0 else np.ones((Bm, heads, Nm, Nm), bool)
    return dict(E=E, S=Sm, A=torch.from_numpy(a).double())


def ones_masks(Bm, Nm, Dm, heads, dtype=torch.float64):
    return dict(E=[torch.ones(Bm * Nm, Dm, dtype=dtype)] * 4, S=[torch.ones(Bm, dtype=dtype)] * 4,
                A=torch.ones(Bm, heads, Nm, Nm, dtype=dtype))


ZERO = dict(E=(0.0, 0.0, 0.0, 0.0), S=0.0, A=0.0)


# ------------------------------------------------------------------ the modules with explicit masks
def _add(x, branch, keepE, p, keepS, p_path, Nm):
    """x + drop_path(dropout(branch)): timm's rule, one keep per sample, kept samples scaled by 1 / (1 - p_path)"""
    return x + branch * keepE / (1.0 - p) * keepS.repeat_interleave(Nm)[:, None] / (1.0 - p_path)


def ffn(sd, x, keepE, p):
    return S.ffn(sd, x) * keepE / (1.0 - p)


def conv_branch(sd, x, Bm, Nm):
    """the ConvModule without its residual and regularisers"""
    t = S.layernorm(x, sd["layer_norm.weight"], sd["layer_norm.bias"], 1e-5)
    u = t @ sd["pointwise_conv1.weight"][:, :, 0].t() + sd["pointwise_conv1.bias"]
    s = S.gn_mixer(u, sd["depthwise_conv.weight"][:, 0], sd["depthwise_conv.bias"], sd["norm.weight"], sd["norm.bias"], Bm, Nm)
    return s @ sd["pointwise_conv2.weight"][:, :, 0].t() + sd["pointwise_conv2.bias"]


def conv_module(sd, x, Bm, Nm, keepE, p, keepS, p_path):
    return _add(x, conv_branch(sd, x, Bm, Nm), keepE, p, keepS, p_path, Nm)


def attention(sd, x, Bm, Nm, heads, keepA, pa):
    """squeezeformer_refs.attention with the dropout on the probabilities; the projection's dropout is the site's"""
    Dm = x.shape[1]
    qkv = (x @ sd["qkv.weight"].t() + sd["qkv.bias"]).view(Bm, Nm, 3, heads, Dm // heads).permute(2, 0, 3, 1, 4)
    pr = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) * (Dm // heads) ** -0.5, -1) * keepA / (1.0 - pa)
    return (pr @ qkv[2]).transpose(1, 2).reshape(Bm * Nm, Dm) @ sd["proj.weight"].t() + sd["proj.bias"]


def block(sd, x, Bm, Nm, heads, squeeze, eps, masks, rates):
    def ln(name, v):
        return S.layernorm(v, sd[name + ".weight"], sd[name + ".bias"], eps)

    def add(i, v, branch):
        return _add(v, branch, masks["E"][i], rates["E"][i], masks["S"][i], rates["S"], Nm)
    x = add(0, x, 0.5 * S.ffn(S._sub(sd, "ffn1."), ln("ffn1_norm", x)))
    x = add(1, x, attention(S._sub(sd, "attn."), ln("attn_norm", x), Bm, Nm, heads, masks["A"], rates["A"]))
    x = add(2, x, conv_branch(S._sub(sd, "conv_module."), x, Bm, Nm))
    if squeeze:
        x = S.se(x, sd["se.fc1.weight"], sd["se.fc1.bias"], sd["se.fc2.weight"], sd["se.fc2.bias"], Bm, Nm)
    x = add(3, x, 0.5 * S.ffn(S._sub(sd, "ffn2."), ln("ffn2_norm", x)))
    return ln("final_norm", x)


def encoder(sd, x, Bm, N0, heads, eps, masks, rates):
    d1 = len({k.split(".")[1] for k in sd if k.startswith("stage1.")})
    d2 = len({k.split(".")[1] for k in sd if k.startswith("stage2.")})
    for i in range(d1):
        x = block(S._sub(sd, f"stage1.{i}."), x, Bm, N0, heads, True, eps, masks[i], rates[i])
    skip, n = x, (N0 // 2 if N0 > 1 else N0)
    x = S.down2(x, Bm, N0)
    for i in range(d2):
        x = block(S._sub(sd, f"stage2.{i}."), x, Bm, n, heads, True, eps, masks[d1 + i], rates[d1 + i])
    x = S.up_add(x, skip, Bm, n, N0)
    return S.layernorm(x, sd["out_norm.weight"], sd["out_norm.bias"], eps)


def run(kind, args, sd, x, eps, masks, rates):
    """the module of kind on x [B][N][D] -> y [B][N][D].  ffn: masks = keepE, rates = p; conv: masks = (keepE, keepS),
    rates = (p, p_path); blocks and the encoder: the dicts (lists of dicts) of the module docstring"""
    Bm, Nm, Dm = x.shape
    r = x.reshape(Bm * Nm, Dm)
    if kind == "ffn":
        y = ffn(sd, r, masks, rates)
    elif kind == "conv":
        y = conv_module(sd, r, Bm, Nm, masks[0], rates[0], masks[1], rates[1])
    elif kind in ("cblock", "sblock"):
        y = block(sd, r, Bm, Nm, args[1], kind == "sblock", eps, masks, rates)
    else:
        y = encoder(sd, r, Bm, Nm, args[1], eps, masks, rates)
    return y.view(Bm, Nm, Dm)


def module_grads(kind, args, sd, x, dy, eps, masks, rates):
    """(y, dx, {parameter name: gradient}) by autograd through `run`"""
    names = [k for k, v in sd.items() if v.is_floating_point()]
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    xr = x.detach().clone().requires_grad_(True)
    y = run(kind, args, leaves, xr, eps, masks, rates)
    grads = torch.autograd.grad((y * dy).sum(), [xr] + list(leaves.values()))
    return y.detach(), grads[0], dict(zip(names, grads[1:]))


# ------------------------------------------------------------------ the two kernels of csrc/dropnorm.hip
def drop_add(x, res, factor):
    """s = res + x * keepE / (1 - p) * keepS / (1 - p_path), factor [rows, D] = the masks times the scales"""
    return res + x * factor


def drop_add_ln_fwd(s, gamma, beta, eps):
    """(y, mean, rstd) from s AS STORED: the LayerNorm half of htrvt_drop_add_ln_fwd"""
    return R.layernorm_fwd(s, gamma, beta, eps)


def layernorm_bwd_drop(dy, s, mean, rstd, gamma, dres, factor):
    """-> ds, dxb, dgamma, dbeta: htrvt_layernorm_bwd's outputs and the branch's gradient dxb = ds * factor"""
    ds, dgamma, dbeta = R.layernorm_bwd(dy, s, mean, rstd, gamma, dres)
    return ds, ds * factor, dgamma, dbeta
