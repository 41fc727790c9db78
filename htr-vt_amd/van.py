"""MI355X-native VANHeightReducer and HorizontalMixer, the two modules the VAN forks put between the ResNet stem (cut
after layer2, a [B, C, 4, W/4] map) and the encoder blocks.

Drop-ins for `LargeKernelAttention(dim)`, `VANBlock(dim, drop_path=0.0)`, `VANHeightReducer(dim, depth=2, drop_path=0.0,
pool="avg")` and `HorizontalMixer(dim, k=9)` of model_sgm_mms_attach_van/model/HTR_VT.py (the copy in
model_sgm_mms_attach_van_2 is identical):
    LargeKernelAttention  u * bn(pw(dwd(dw(u))))           dw 5x5 depthwise, dwd 7x7 depthwise dilation 3, pw 1x1
    VANBlock              x + norm(proj2(lka(gelu(proj1(x)))))
    VANHeightReducer      the blocks, then the mean over the height: (B, C, H, W) -> (B, C, 1, W)
    HorizontalMixer       gelu(x + bn(pw(dw(x))))          dw 1xk depthwise along the width, on (B, C, 1, W)
Same module tree, names, shapes and construction order as the fork's, so `torch.manual_seed(s)` followed by a constructor
gives the fork's initial state_dict and a fork checkpoint's `van_reducer.*` / `hmix.*` entries load with strict=True.

Every step is a HIP kernel: the 1x1 convolutions and their gradients on the GEMM / column-sum kernels, the BatchNorm
statistics and backward on the htrvt_bn_* passes, the depthwise convolutions, the LKA gate, BatchNorm + shortcut + GELU and
the height pool on csrc/van.hip, all through the launch sequences of seq_ops.  Activations are NHWC: the reducer converts
its input once at the entry and its output once at the exit, not per block.  One autograd node per VANBlock, one for the
pool, one for HorizontalMixer.  The gradients are bitwise reproducible (no float atomics).  Train mode uses the batch
statistics and updates the BatchNorm buffers in place (num_batches_tracked included); eval mode reads them and leaves
them untouched.
compute_dtype: torch.float32 (parity) or torch.bfloat16 (activations and GEMM operands; BatchNorm statistics and every
parameter gradient stay float32).  Inputs (any memory format) and outputs are float32.  dim a multiple of 8.
Not served, as the forks build neither: pool="max", and drop_path > 0 in train mode (NotImplementedError).
"""
import torch
import torch.nn as nn

from . import seq_ops
from .seq_ops import convert as _convert

BLOCK_PARAMS = ("proj1.weight", "proj1.bias", "lka.dw.weight", "lka.dwd.weight", "lka.pw.weight", "lka.bn.weight",
                "lka.bn.bias", "proj2.weight", "proj2.bias", "norm.weight", "norm.bias")
LKA_PARAMS = ("dw.weight", "dwd.weight", "pw.weight", "bn.weight", "bn.bias")
MIXER_PARAMS = ("dw.weight", "pw.weight", "bn.weight", "bn.bias")


def _as(t, dtype):
    """t (contiguous) in dtype: itself, or a converted copy"""
    return t if t.dtype == dtype else _convert(t, torch.empty(t.shape, dtype=dtype, device=t.device))


def _nhwc(x, cdt):
    """(B, C, H, W) in any memory format -> contiguous [B, H, W, C] in the compute dtype"""
    return _as(x.permute(0, 2, 3, 1).contiguous().float(), cdt)


def _nchw(y):
    """[B, H, W, C] -> float32 (B, C, H, W) over the same memory (channels last)"""
    return _as(y, torch.float32).permute(0, 3, 1, 2)


def _bn(bn):
    return (bn.weight.contiguous(), bn.bias.contiguous(), bn.running_mean, bn.running_var, bn.num_batches_tracked)


def _params(names, params, cdt):
    """by name; the 1x1 convolution weights [C, C, 1, 1] as [C, C] in the compute dtype"""
    P = {n: t.contiguous() for n, t in zip(names, params)}
    for n, t in P.items():
        if t.dim() == 4 and t.shape[-2:] == (1, 1) and t.shape[1] != 1:
            P[n] = _as(t.view(t.shape[0], t.shape[1]), cdt)
    return P


def _grads(names, grads, shapes):
    return tuple(grads[n].view(s) for n, s in zip(names, shapes))


def _check_input(mod, x, dim, params, height=None):
    name = type(mod).__name__
    if not all(t.is_cuda for t in [x] + list(params)):
        raise RuntimeError(f"{name} runs on an MI355X only: move the module and its input to cuda "
                           "(no CPU / eager fallback exists)")
    if x.dim() != 4 or x.shape[1] != dim or (height is not None and x.shape[2] != height):
        raise ValueError(f"{name}: x (B, {dim}, {'H' if height is None else height}, W) expected, got {tuple(x.shape)}")


def _need(x, params):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))


def _check_ctor(name, dim, compute_dtype):
    if dim % 8 or dim < 8:
        raise ValueError(f"{name}: dim a multiple of 8, got {dim}")
    if compute_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name}: compute_dtype torch.float32 or torch.bfloat16, got {compute_dtype}")


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cdt):
        return _nhwc(x, cdt)

    @staticmethod
    def backward(ctx, dy):
        return _nchw(dy.contiguous()), None


class _FromNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y):
        ctx.cdt = y.dtype
        return _nchw(y)

    @staticmethod
    def backward(ctx, dy):
        return _nhwc(dy, ctx.cdt)


class _LKAFunction(torch.autograd.Function):
    """a [B, H, W, C] -> a * bn(pw(dwd(dw(a))))"""

    @staticmethod
    def forward(ctx, mod, a, need, *params):
        P = _params(LKA_PARAMS, params, a.dtype)
        g, saved = seq_ops.lka_fwd(a, P["dw.weight"], P["dwd.weight"], P["pw.weight"], _bn(mod.bn), mod.training, mod.bn.eps,
                                   mod.bn.momentum)
        g = g.view(a.shape)
        if need:
            ctx.save_for_backward(a, *[P[n] for n in LKA_PARAMS], *saved)
            ctx.training, ctx.shapes = mod.training, [p.shape for p in params]
        else:
            ctx.mark_non_differentiable(g)
        return g

    @staticmethod
    def backward(ctx, dg):
        a, *rest = ctx.saved_tensors
        P, saved = dict(zip(LKA_PARAMS, rest)), rest[len(LKA_PARAMS):]
        C = a.shape[-1]
        da, grads = seq_ops.lka_bwd(dg.contiguous().view(-1, C), a, P["dw.weight"], P["dwd.weight"], P["pw.weight"],
                                    P["bn.weight"], saved, ctx.training)
        return (None, da, None) + _grads(LKA_PARAMS, grads, ctx.shapes)


class _BlockFunction(torch.autograd.Function):
    """x [B, H, W, C] in the compute dtype -> the VANBlock's output, same layout"""

    @staticmethod
    def forward(ctx, mod, x, need, *params):
        P = _params(BLOCK_PARAMS, params, x.dtype)
        y, saved = seq_ops.van_block_fwd(x, P, _bn(mod.lka.bn), _bn(mod.norm), mod.training, (mod.lka.bn.eps, mod.norm.eps),
                                         (mod.lka.bn.momentum, mod.norm.momentum))
        if need:
            ctx.save_for_backward(x, *[P[n] for n in BLOCK_PARAMS], *saved)
            ctx.training, ctx.shapes = mod.training, [p.shape for p in params]
        else:
            ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, *rest = ctx.saved_tensors
        P, saved = dict(zip(BLOCK_PARAMS, rest)), rest[len(BLOCK_PARAMS):]
        dx, grads = seq_ops.van_block_bwd(dy.contiguous(), x, P, saved, ctx.training)
        return (None, dx, None) + _grads(BLOCK_PARAMS, grads, ctx.shapes)


class _PoolFunction(torch.autograd.Function):
    """[B, H, W, C] in the compute dtype -> float32 (B, C, 1, W), the mean over H"""

    @staticmethod
    def forward(ctx, x):
        ctx.geo = (x.shape[1], x.dtype)
        return _nchw(seq_ops.height_pool_fwd(x).unsqueeze(1))

    @staticmethod
    def backward(ctx, dy):
        H, cdt = ctx.geo
        return seq_ops.height_pool_bwd(_nhwc(dy, cdt).squeeze(1), H)


class _MixerFunction(torch.autograd.Function):
    """float32 (B, C, 1, W) -> gelu(x + bn(pw(dw(x)))), float32 (B, C, 1, W)"""

    @staticmethod
    def forward(ctx, mod, x, need, *params):
        cdt = mod.compute_dtype
        P = _params(MIXER_PARAMS, params, cdt)
        xh = _nhwc(x, cdt)
        y, saved = seq_ops.hmixer_fwd(xh, P["dw.weight"], P["pw.weight"], _bn(mod.bn), mod.training, mod.bn.eps, mod.bn.momentum)
        y = _nchw(y)
        if need:
            ctx.save_for_backward(xh, *[P[n] for n in MIXER_PARAMS], *saved)
            ctx.training, ctx.shapes = mod.training, [p.shape for p in params]
        else:
            ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        xh, *rest = ctx.saved_tensors
        P, saved = dict(zip(MIXER_PARAMS, rest)), rest[len(MIXER_PARAMS):]
        dx, grads = seq_ops.hmixer_bwd(_nhwc(dy, xh.dtype), xh, P["dw.weight"], P["pw.weight"], P["bn.weight"], saved,
                                       ctx.training)
        return (None, _nchw(dx), None) + _grads(MIXER_PARAMS, grads, ctx.shapes)


class LargeKernelAttention(nn.Module):
    """depthwise 5x5, depthwise 7x7 dilation 3, pointwise 1x1, BatchNorm; the result gates the input"""

    def __init__(self, dim, compute_dtype=torch.float32):
        super().__init__()
        _check_ctor("LargeKernelAttention", dim, compute_dtype)
        self.dw = nn.Conv2d(dim, dim, kernel_size=5, padding=2, groups=dim, bias=False)
        self.dwd = nn.Conv2d(dim, dim, kernel_size=7, padding=9, dilation=3, groups=dim, bias=False)
        self.pw = nn.Conv2d(dim, dim, kernel_size=1, bias=False)
        self.bn = nn.BatchNorm2d(dim)
        self.compute_dtype = compute_dtype

    def forward(self, x):
        params = [self.get_parameter(n) for n in LKA_PARAMS]
        _check_input(self, x, self.pw.in_channels, params)
        with torch.cuda.device(x.device):
            a = _ToNHWC.apply(x, self.compute_dtype)
            return _FromNHWC.apply(_LKAFunction.apply(self, a, _need(x, params), *params))


class VANBlock(nn.Module):
    """1x1 -> GELU -> LKA -> 1x1 -> BatchNorm, + shortcut"""

    def __init__(self, dim, drop_path=0.0, compute_dtype=torch.float32):
        super().__init__()
        _check_ctor("VANBlock", dim, compute_dtype)
        self.proj1 = nn.Conv2d(dim, dim, kernel_size=1, bias=True)
        self.act = nn.GELU()
        self.lka = LargeKernelAttention(dim, compute_dtype)
        self.proj2 = nn.Conv2d(dim, dim, kernel_size=1, bias=True)
        self.norm = nn.BatchNorm2d(dim)
        self.drop_path = nn.Identity()
        self.drop_path_rate = float(drop_path)
        self.compute_dtype = compute_dtype

    def forward_nhwc(self, x, need=None):
        """x [B, H, W, C] in the compute dtype -> the same layout: the block without the layout conversions"""
        if self.training and self.drop_path_rate > 0:
            raise NotImplementedError("VANBlock: drop_path > 0 in train mode is not served (the forks build 0.0)")
        params = [self.get_parameter(n) for n in BLOCK_PARAMS]
        return _BlockFunction.apply(self, x, _need(x, params) if need is None else need, *params)

    def forward(self, x):
        params = [self.get_parameter(n) for n in BLOCK_PARAMS]
        _check_input(self, x, self.proj1.in_channels, params)
        with torch.cuda.device(x.device):
            return _FromNHWC.apply(self.forward_nhwc(_ToNHWC.apply(x, self.compute_dtype), _need(x, params)))


class VANHeightReducer(nn.Module):
    """a few VANBlocks, then the height collapsed to 1 by its mean: (B, C, H, W) -> (B, C, 1, W)"""

    def __init__(self, dim, depth=2, drop_path=0.0, pool="avg", compute_dtype=torch.float32):
        super().__init__()
        _check_ctor("VANHeightReducer", dim, compute_dtype)
        if pool == "max":
            raise NotImplementedError("VANHeightReducer: pool='max' is not served (the forks build 'avg')")
        if pool != "avg":
            raise ValueError(f"Unsupported pool type: {pool}")
        self.blocks = nn.Sequential(*[VANBlock(dim, drop_path=drop_path, compute_dtype=compute_dtype) for _ in range(depth)])
        self.pool = nn.AdaptiveAvgPool2d((1, None))
        self.compute_dtype = compute_dtype

    def forward(self, x):
        params = list(self.parameters())
        _check_input(self, x, self.blocks[0].proj1.in_channels if len(self.blocks) else x.shape[1], params)
        need = _need(x, params)
        with torch.cuda.device(x.device):
            t = _ToNHWC.apply(x, self.compute_dtype)
            for blk in self.blocks:
                t = blk.forward_nhwc(t, need)
            return _PoolFunction.apply(t)


class HorizontalMixer(nn.Module):
    """depthwise 1xk along the width -> 1x1 -> BatchNorm, + shortcut, GELU; (B, C, 1, W) keeps its shape"""

    def __init__(self, dim, k=9, compute_dtype=torch.float32):
        super().__init__()
        _check_ctor("HorizontalMixer", dim, compute_dtype)
        if k % 2 != 1 or not 1 <= k <= 9:
            raise ValueError(f"HorizontalMixer: k odd, 1 ... 9, got {k}")
        self.dw = nn.Conv2d(dim, dim, kernel_size=(1, k), padding=(0, k // 2), groups=dim, bias=False)
        self.pw = nn.Conv2d(dim, dim, kernel_size=1, bias=False)
        self.bn = nn.BatchNorm2d(dim)
        self.act = nn.GELU()
        self.compute_dtype = compute_dtype

    def forward(self, x):
        params = [self.get_parameter(n) for n in MIXER_PARAMS]
        _check_input(self, x, self.pw.in_channels, params, height=1)
        with torch.cuda.device(x.device):
            return _MixerFunction.apply(self, x, _need(x, params), *params)
