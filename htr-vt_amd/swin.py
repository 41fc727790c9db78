"""MI355X-native blocks of the Swin fork (model_sgm_mms_swin/model/HTR_VT.py): the four modules its HTR_VT_Swin builds its
three stages from, on the 4 x 128, 2 x 128 and 1 x 128 token maps behind the ResNet stem.

Drop-ins for
    WindowAttention2D(dim, num_heads, window_size)        qkv, attention with the learned relative-position bias, proj
    SwinBlock2D(dim, num_heads, window_size, shift_size, mlp_ratio=4.0, drop=0.0)
                                                          x + attn(norm1(x)) in (shifted) windows, then x + mlp(norm2(x))
    HeightOnlyPatchMerging(in_dim, out_dim)               Conv2d (2, 1) stride (2, 1) over the height, LayerNorm
    Combining(in_dim, out_dim, drop=0.1)                  mean over the height, Linear, GELU
and the helpers window_partition / window_reverse as plain torch.  Same module tree, names, shapes and construction order as
the fork's, so `torch.manual_seed(s)` followed by a constructor gives the fork's initial state_dict (the table's
trunc_normal_ included) and a fork checkpoint's entries load with strict=True.

Every arithmetic step is a HIP kernel: the attention is csrc/swin.hip (roll, window partition, bias, the fork's two-region
additive -100 mask, window reverse and roll-back inside one kernel on token-order qkv), the rest are the LayerNorm, GEMM,
column-sum, GELU-backward and height-pool kernels through the launch sequences of seq_ops.  What torch does is copies: the
input made contiguous float32 at a module's entry, and in HeightOnlyPatchMerging the strided gather of the even / odd map rows
(forward) and the two torch.stack interleaves of its backward (the input gradient's row planes, the weight gradient's taps).  One autograd node per SwinBlock2D, one per
HeightOnlyPatchMerging, one per Combining.  The gradients are bitwise reproducible (no float atomics).  The blocks have no
train-only state at drop=0: eval equals train.
compute_dtype: torch.float32 (parity) or torch.bfloat16 (activations and GEMM operands; every parameter gradient stays
float32).  Inputs and outputs are float32.
Not served: drop > 0 in train mode (the fork's create_model builds 0.0; eval mode is the identity and is served), an odd
height in HeightOnlyPatchMerging (the fork merges 4 -> 2 -> 1), an attn_mask handed to WindowAttention2D (the block does not
go through it: its mask is inside the kernel), head widths other than 32 / 64 / 128 and windows of more than 32 tokens.
"""
import torch
import torch.nn as nn

from . import seq_ops
from .seq_ops import convert as _convert

ATTN_PARAMS = ("relative_position_bias_table", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias")
BLOCK_PARAMS = ("norm1.weight", "norm1.bias") + tuple("attn." + n for n in ATTN_PARAMS) + (
    "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")
MERGE_PARAMS = ("reduce.weight", "norm.weight", "norm.bias")
COMBINE_PARAMS = ("fc.weight", "fc.bias")
HEAD_DIMS = (32, 64, 128)
MAX_WINDOW = 32


def window_partition(x, wh, ww):
    """x [B, H, W, C] -> [B * (H / wh) * (W / ww), wh * ww, C]"""
    B, H, W, C = x.shape
    x = x.view(B, H // wh, wh, W // ww, ww, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, wh * ww, C)


def window_reverse(windows, wh, ww, H, W, B):
    """[B * (H / wh) * (W / ww), wh * ww, C] -> [B, H, W, C]"""
    x = windows.view(B, H // wh, W // ww, wh, ww, -1).permute(0, 1, 3, 2, 4, 5).contiguous()
    return x.view(B, H, W, -1)


def _as(t, dtype):
    """t (contiguous) in dtype: itself, or a converted copy"""
    return t if t.dtype == dtype else _convert(t, torch.empty(t.shape, dtype=dtype, device=t.device))


def _rows(x, cdt):
    """x [B, N, C] float32, any strides -> contiguous rows [B*N, C] in the compute dtype"""
    return _as(x.contiguous().float().view(-1, x.shape[-1]), cdt)


def _params(names, params, cdt):
    """by name; the Linear weights [out, in] in the compute dtype, the (2, 1) convolution's weight as its two [out, in] taps"""
    P = {n: t.contiguous() for n, t in zip(names, params)}
    for n, t in P.items():
        if t.dim() == 2 and not n.endswith("relative_position_bias_table"):
            P[n] = _as(t, cdt)
        elif t.dim() == 4:
            P[n] = (_as(t[:, :, 0, 0].contiguous(), cdt), _as(t[:, :, 1, 0].contiguous(), cdt))
    return P


def _grads(names, grads, shapes):
    return tuple(grads[n].view(s) for n, s in zip(names, shapes))


def _need(x, params):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))


def _check_device(mod, x, params):
    if not all(t.is_cuda for t in [x] + list(params)):
        raise RuntimeError(f"{type(mod).__name__} runs on an MI355X only: move the module and its input to cuda "
                           "(no CPU / eager fallback exists)")


def _check_tokens(mod, x, H, W, dim):
    if x.dim() != 3 or x.shape[2] != dim:
        raise ValueError(f"{type(mod).__name__}: x (B, N, {dim}) expected, got {tuple(x.shape)}")
    if x.shape[1] != H * W:
        raise ValueError(f"{type(mod).__name__}: N = {x.shape[1]} tokens are not the H * W = {H} * {W} map")


def _check_dtype(name, compute_dtype):
    if compute_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name}: compute_dtype torch.float32 or torch.bfloat16, got {compute_dtype}")


def _check_attention(name, dim, num_heads, window_size):
    if num_heads < 1 or dim % num_heads:
        raise ValueError(f"{name}: dim {dim} is not a multiple of num_heads {num_heads}")
    if dim // num_heads not in HEAD_DIMS:
        raise ValueError(f"{name}: head width {dim // num_heads} (dim / num_heads) outside {HEAD_DIMS}")
    wh, ww = window_size
    if wh < 1 or ww < 1 or wh * ww > MAX_WINDOW:
        raise ValueError(f"{name}: window {wh} x {ww} outside 1 ... {MAX_WINDOW} tokens")


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
            flat = [t for n in names for t in (P[n] if isinstance(P[n], tuple) else (P[n],))]
            ctx.save_for_backward(xr, *flat, *saved)
            ctx.mod, ctx.geo, ctx.nsaved = mod, geo, len(saved)
            ctx.shapes, ctx.xshape = [p.shape for p in params], x.shape
        else:
            ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        mod = ctx.mod
        xr, *rest = ctx.saved_tensors
        flat, saved = rest[:len(rest) - ctx.nsaved], rest[len(rest) - ctx.nsaved:]
        P, it = {}, iter(flat)
        for n, s in zip(mod.PARAMS, ctx.shapes):
            P[n] = (next(it), next(it)) if len(s) == 4 else next(it)
        dyr = _as(dy.contiguous().float().view(-1, dy.shape[-1]), xr.dtype)
        dx, grads = mod._bwd(dyr, xr, P, saved, ctx.geo)
        return (None, None, _as(dx, torch.float32).view(ctx.xshape), None) + _grads(mod.PARAMS, grads, ctx.shapes)


class WindowAttention2D(nn.Module):
    """qkv Linear, attention inside one wh x ww window per row of the batch with the learned relative-position bias, proj"""
    PARAMS = ATTN_PARAMS

    def __init__(self, dim, num_heads, window_size, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("WindowAttention2D", compute_dtype)
        _check_attention("WindowAttention2D", dim, num_heads, window_size)
        self.dim = dim
        self.num_heads = num_heads
        self.wh, self.ww = window_size
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * self.wh - 1) * (2 * self.ww - 1), num_heads))
        # the table entry of (query slot t, key slot u), slot = r * ww + c: the kernel's own index (include/htrvt.h)
        t = torch.arange(self.wh * self.ww)
        r, c = t // self.ww, t % self.ww
        self.register_buffer("relative_position_index", (r[:, None] - r[None, :] + self.wh - 1) * (2 * self.ww - 1)
                             + (c[:, None] - c[None, :] + self.ww - 1))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.compute_dtype = compute_dtype

    def _fwd(self, xr, P, xshape, hw, need):
        y, saved = seq_ops.window_attention_fwd(xr, P, xshape[0], self.num_heads, (self.wh, self.ww))
        return y, saved, xshape[0], xshape

    def _bwd(self, dy, xr, P, saved, Bn):
        return seq_ops.window_attention_bwd(dy, xr, P, saved, Bn, self.num_heads, (self.wh, self.ww))

    def forward(self, x, attn_mask=None):
        """x [num_windows * B, wh * ww, C], partitioned windows"""
        _check_tokens(self, x, self.wh, self.ww, self.dim)
        if attn_mask is not None:
            raise NotImplementedError("WindowAttention2D: an attn_mask is not served on the device (SwinBlock2D's mask is "
                                      "inside its attention kernel)")
        params = [self.get_parameter(n) for n in self.PARAMS]
        _check_device(self, x, params)
        with torch.cuda.device(x.device):
            return _Function.apply(self, None, x, _need(x, params), *params)


class SwinBlock2D(nn.Module):
    """x + attn(norm1(x)) inside (shifted) windows, then x + mlp(norm2(x))"""
    PARAMS = BLOCK_PARAMS

    def __init__(self, dim, num_heads, window_size, shift_size, mlp_ratio=4.0, drop=0.0, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("SwinBlock2D", compute_dtype)
        _check_attention("SwinBlock2D", dim, num_heads, window_size)
        self.dim = dim
        self.wh, self.ww = window_size
        self.sh, self.sw = shift_size
        if not (0 <= self.sh < self.wh and 0 <= self.sw < self.ww):
            raise ValueError(f"SwinBlock2D: shift {tuple(shift_size)} outside its window {tuple(window_size)}")
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention2D(dim, num_heads, window_size, compute_dtype=compute_dtype)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = nn.Sequential(
            nn.Linear(dim, int(dim * mlp_ratio)),
            nn.GELU(),
            nn.Dropout(drop),
            nn.Linear(int(dim * mlp_ratio), dim),
            nn.Dropout(drop),
        )
        self.drop = float(drop)
        self.compute_dtype = compute_dtype

    def _fwd(self, xr, P, xshape, hw, need):
        geo = (xshape[0],) + hw
        y, saved = seq_ops.swin_block_fwd(xr, P, *geo, self.attn.num_heads, (self.wh, self.ww), (self.sh, self.sw),
                                          self.norm1.eps, save=need)
        return y, saved if need else (), geo, xshape

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.swin_block_bwd(dy, xr, P, saved, *geo, self.attn.num_heads, (self.wh, self.ww), (self.sh, self.sw))

    def forward(self, x, H, W):
        """x [B, H * W, C] -> the same shape"""
        _check_tokens(self, x, H, W, self.dim)
        if H % self.wh or W % self.ww:
            raise ValueError(f"SwinBlock2D: map {H} x {W} is not a whole number of {self.wh} x {self.ww} windows")
        if self.training and self.drop > 0:
            raise NotImplementedError("SwinBlock2D: drop > 0 in train mode is not served (the fork builds 0.0)")
        params = [self.get_parameter(n) for n in self.PARAMS]
        _check_device(self, x, params)
        with torch.cuda.device(x.device):
            return _Function.apply(self, (H, W), x, _need(x, params), *params)


class HeightOnlyPatchMerging(nn.Module):
    """Conv2d(in, out, (2, 1), stride (2, 1), bias=False) over the token map, LayerNorm: [B, H * W, in] -> [B, H/2 * W, out]"""
    PARAMS = MERGE_PARAMS

    def __init__(self, in_dim, out_dim, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("HeightOnlyPatchMerging", compute_dtype)
        self.reduce = nn.Conv2d(in_dim, out_dim, kernel_size=(2, 1), stride=(2, 1), bias=False)
        self.norm = nn.LayerNorm(out_dim)
        self.compute_dtype = compute_dtype

    def _fwd(self, xr, P, xshape, hw, need):
        geo = (xshape[0],) + hw
        y, saved = seq_ops.patch_merge_fwd(xr, P, *geo, self.norm.eps, save=need)
        return y, saved if need else (), geo, (xshape[0], geo[1] // 2 * geo[2], y.shape[1])

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.patch_merge_bwd(dy, P, saved, *geo)

    def forward(self, x, H, W):
        """x [B, H * W, C] -> (x [B, H/2 * W, out], H/2, W)"""
        _check_tokens(self, x, H, W, self.reduce.in_channels)
        if H % 2:
            raise NotImplementedError(f"HeightOnlyPatchMerging: an odd height {H} is not served (the fork merges 4 -> 2 -> 1)")
        params = [self.get_parameter(n) for n in self.PARAMS]
        _check_device(self, x, params)
        with torch.cuda.device(x.device):
            return _Function.apply(self, (H, W), x, _need(x, params), *params), H // 2, W


class Combining(nn.Module):
    """mean over the height, Linear, GELU: [B, H * W, in] -> [B, W, out]"""
    PARAMS = COMBINE_PARAMS

    def __init__(self, in_dim, out_dim, drop=0.1, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("Combining", compute_dtype)
        self.fc = nn.Linear(in_dim, out_dim)
        self.act = nn.GELU()
        self.drop = nn.Dropout(drop)
        self.compute_dtype = compute_dtype

    def _fwd(self, xr, P, xshape, hw, need):
        geo = (xshape[0],) + hw
        y, saved = seq_ops.combining_fwd(xr, P, *geo)
        return y, saved if need else (), geo, (xshape[0], geo[2], y.shape[1])

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.combining_bwd(dy, P, saved, *geo)

    def forward(self, x, H, W):
        """x [B, H * W, C] -> [B, W, out]"""
        _check_tokens(self, x, H, W, self.fc.in_features)
        if self.training and self.drop.p > 0:
            raise NotImplementedError("Combining: drop > 0 in train mode is not served (the fork builds 0.0)")
        params = [self.get_parameter(n) for n in self.PARAMS]
        _check_device(self, x, params)
        with torch.cuda.device(x.device):
            return _Function.apply(self, (H, W), x, _need(x, params), *params)
