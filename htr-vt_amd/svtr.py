"""MI355X-native mixing blocks of the SVTR fork (model_sgm_mms_svtr/model/svtr.py): the modules its SVTR encoder builds its
three stages from, on the 16 x 128, 8 x 128 and 4 x 128 token maps behind its patch embedding.

Drop-ins for
    MultiHeadSelfAttention(dim, num_heads=8, local=False, local_k=(7, 11))    qkv (no bias), attention, proj
    MixingBlock(dim, num_heads=8, local=False)             x + attn(norm1(x)), then x + mlp(norm2(x))
    Merging(in_dim, out_dim)                               Conv2d 3x3 stride (2, 1) padding 1 over the map, LayerNorm
    Combining(in_dim, out_dim, drop=0.1)                   mean over the height, Linear, GELU: the Swin fork's, re-exported
Same module tree, attribute names (local, local_k, num_heads, head_dim, scale), state_dict keys and construction order as
the fork's, so `torch.manual_seed(s)` followed by a constructor gives the fork's initial state_dict and a fork checkpoint's
entries load with strict=True.  No buffers: the fork's cached `mask` attribute is not state and is not reproduced.

A local module attends inside the centred local_k = (kh, kw) box of the token map: csrc/svtr.hip, the neighbourhood kernel on
token-order qkv (the fork builds dense N x N scores and adds a -inf mask).  A global module in bfloat16 runs the fused
attention kernel of csrc/attention.hip; in float32, and in bfloat16 on maps of fewer than 32 tokens, the unfused GEMM route,
which keeps a [B * heads, N, N] P and needs N a multiple of 8 (4 in float32): the parity route, not a training one.  Merging
gathers its convolution inside htrvt_gemm (the NHWC map is the token rows as they are); the weight's repacking and the
weight gradient's way back are torch copies.  Everything else is the LayerNorm, GEMM, column-sum, GELU-backward and
height-pool kernels through the launch sequences of seq_ops.  One autograd node per MixingBlock, per Merging, per Combining
and per stand-alone MultiHeadSelfAttention; every parameter gradient is float32; the gradients are bitwise reproducible.
compute_dtype: torch.float32 (parity) or torch.bfloat16.  Inputs and outputs are float32.
Not served: head widths other than 32 / 64, an even local_k or one beyond (7, 11), N != H * W (the fork's fallback branch
for that case builds a mask that masks nothing), Combining's drop > 0 in train mode.
"""
import torch
import torch.nn as nn

from . import seq_ops
from .swin import Combining, _as, _check_device, _check_dtype, _check_tokens, _grads, _need, _rows

__all__ = ["MultiHeadSelfAttention", "MixingBlock", "Merging", "Combining"]

ATTN_PARAMS = ("qkv.weight", "proj.weight", "proj.bias")
BLOCK_PARAMS = ("norm1.weight", "norm1.bias") + tuple("attn." + n for n in ATTN_PARAMS) + (
    "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias")
MERGE_PARAMS = ("conv.weight", "conv.bias", "norm.weight", "norm.bias")
HEAD_DIMS = (32, 64)
MAX_LOCAL_K = (7, 11)


def _params(names, params, cdt):
    """by name; the Linear weights [out, in] in the compute dtype, the 3x3 convolution's weight as its (forward, dgrad)
    packs, everything else float32 as stored"""
    P = {n: t.contiguous() for n, t in zip(names, params)}
    for n, t in P.items():
        if t.dim() == 2:
            P[n] = _as(t, cdt)
        elif t.dim() == 4:
            P[n] = seq_ops.svtr_merge_packs(t.float(), cdt)
    return P


def _check_attention(name, dim, num_heads, local, local_k):
    if num_heads < 1 or dim % num_heads:
        raise ValueError(f"{name}: dim {dim} is not a multiple of num_heads {num_heads}")
    if dim // num_heads not in HEAD_DIMS:
        raise ValueError(f"{name}: head width {dim // num_heads} (dim / num_heads) outside {HEAD_DIMS}")
    if local:
        kh, kw = local_k
        if kh < 1 or kw < 1 or kh % 2 == 0 or kw % 2 == 0 or kh > MAX_LOCAL_K[0] or kw > MAX_LOCAL_K[1]:
            raise ValueError(f"{name}: local_k {tuple(local_k)}: odd sides, at most {MAX_LOCAL_K}")


class _Function(torch.autograd.Function):
    """one node for a whole module: forward(mod, (H, W), x, need, *params) over mod._fwd / mod._bwd, the seq_ops sequences"""

    @staticmethod
    def forward(ctx, mod, hw, x, need, *params):
        names = mod.PARAMS
        P = _params(names, params, mod.compute_dtype)
        xr = _rows(x, mod.compute_dtype)
        y, saved, geo, out_shape = mod._fwd(xr, P, x.shape, hw, need)
        y = _as(y, torch.float32).view(out_shape)
        if need:
            saved = tuple(saved)
            ctx.none = [t is None for t in saved]
            flat = [t for n in names for t in (P[n] if isinstance(P[n], tuple) else (P[n],))]
            ctx.save_for_backward(xr, *flat, *[t for t in saved if t is not None])
            ctx.mod, ctx.geo, ctx.nsaved = mod, geo, sum(not z for z in ctx.none)
            ctx.shapes, ctx.xshape = [p.shape for p in params], x.shape
        else:
            ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        mod = ctx.mod
        xr, *rest = ctx.saved_tensors
        flat, kept = rest[:len(rest) - ctx.nsaved], iter(rest[len(rest) - ctx.nsaved:])
        saved = tuple(None if z else next(kept) for z in ctx.none)
        P, it = {}, iter(flat)
        for n, s in zip(mod.PARAMS, ctx.shapes):
            P[n] = (next(it), next(it)) if len(s) == 4 else next(it)
        dyr = _as(dy.contiguous().float().view(-1, dy.shape[-1]), xr.dtype)
        dx, grads = mod._bwd(dyr, xr, P, saved, ctx.geo)
        return (None, None, _as(dx, torch.float32).view(ctx.xshape), None) + _grads(mod.PARAMS, grads, ctx.shapes)


def _apply(mod, x, H, W):
    params = [mod.get_parameter(n) for n in mod.PARAMS]
    _check_device(mod, x, params)
    with torch.cuda.device(x.device):
        return _Function.apply(mod, (H, W), x, _need(x, params), *params)


class MultiHeadSelfAttention(nn.Module):
    """qkv Linear (no bias), attention over the whole map (local=False) or inside the centred local_k box, proj"""
    PARAMS = ATTN_PARAMS

    def __init__(self, dim, num_heads=8, local=False, local_k=(7, 11), compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("MultiHeadSelfAttention", compute_dtype)
        _check_attention("MultiHeadSelfAttention", dim, num_heads, local, local_k)
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.proj = nn.Linear(dim, dim)
        self.local = local
        self.local_k = local_k
        self.compute_dtype = compute_dtype

    @property
    def kernel(self):
        """(kh, kw) of a local module, None of a global one: what the seq_ops sequences take"""
        return tuple(int(k) for k in self.local_k) if self.local else None

    def _fwd(self, xr, P, xshape, hw, need):
        geo = (xshape[0],) + hw
        y, saved = seq_ops.mha_fwd(xr, P, *geo, self.num_heads, self.kernel, save=need)
        return y, saved if need else (), geo, xshape

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.mha_bwd(dy, xr, P, saved, *geo, self.num_heads, self.kernel)

    def forward(self, x, H, W):
        """x [B, H * W, C] -> the same shape"""
        _check_tokens(self, x, H, W, self.qkv.in_features)
        return _apply(self, x, H, W)


class MixingBlock(nn.Module):
    """x + attn(norm1(x)), local or global, then x + mlp(norm2(x))"""
    PARAMS = BLOCK_PARAMS

    def __init__(self, dim, num_heads=8, local=False, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("MixingBlock", compute_dtype)
        _check_attention("MixingBlock", dim, num_heads, local, MAX_LOCAL_K)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = MultiHeadSelfAttention(dim, num_heads, local=local, compute_dtype=compute_dtype)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = nn.Sequential(
            nn.Linear(dim, dim * 4),
            nn.GELU(),
            nn.Linear(dim * 4, dim)
        )
        self.compute_dtype = compute_dtype

    def _fwd(self, xr, P, xshape, hw, need):
        geo = (xshape[0],) + hw
        y, saved = seq_ops.mixing_block_fwd(xr, P, *geo, self.attn.num_heads, self.attn.kernel, self.norm1.eps, save=need)
        return y, saved if need else (), geo, xshape

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.mixing_block_bwd(dy, xr, P, saved, *geo, self.attn.num_heads, self.attn.kernel)

    def forward(self, x, H, W):
        """x [B, H * W, C] -> the same shape"""
        _check_tokens(self, x, H, W, self.norm1.normalized_shape[0])
        return _apply(self, x, H, W)


class Merging(nn.Module):
    """Conv2d(in, out, 3, stride (2, 1), padding 1) over the token map, LayerNorm: [B, H * W, in] -> [B, Ho * W, out] with
    Ho = (H - 1) // 2 + 1"""
    PARAMS = MERGE_PARAMS

    def __init__(self, in_dim, out_dim, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("Merging", compute_dtype)
        self.conv = nn.Conv2d(in_dim, out_dim, kernel_size=3, stride=(2, 1), padding=1)
        self.norm = nn.LayerNorm(out_dim)
        self.compute_dtype = compute_dtype

    def _fwd(self, xr, P, xshape, hw, need):
        geo = (xshape[0],) + hw
        y, saved = seq_ops.svtr_merge_fwd(xr, P, *geo, self.norm.eps, save=need)
        return y, saved if need else (), geo, (xshape[0], ((hw[0] - 1) // 2 + 1) * hw[1], y.shape[1])

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.svtr_merge_bwd(dy, xr, P, saved, *geo)

    def forward(self, x, H, W):
        """x [B, H * W, C] -> (x [B, Ho * W, out], Ho, W)"""
        _check_tokens(self, x, H, W, self.conv.in_channels)
        return _apply(self, x, H, W), (H - 1) // 2 + 1, W
