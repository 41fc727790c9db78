"""MI355X-native ConvLocalMixer1D, the convolutional token mixer of the macaron forks.

Drop-in for `ConvLocalMixer1D(dim, kernel_size=7, drop=0.1, use_bn=True)` of model_sgm_macaron/model/HTR_VT.py (the copy
in model_sgm_macaron_2 is identical): for x [B, N, D]
    x + dropout(pw_out(silu(bn(dwconv(glu(pw_in(LayerNorm(x))))))))
Same module tree, names, shapes and construction order as the fork's, so `torch.manual_seed(s); ConvLocalMixer1D(...)`
gives its initial state_dict.  The forward is ONE autograd node over HIP kernels: LayerNorm (eps 1e-5), the two Linear
layers and their gradients on the GEMM / column-sum kernels of the hot path, GLU + depthwise convolution along the tokens
+ BatchNorm1d + SiLU on csrc/mixer.hip through seq_ops.conv_mixer_fwd / _bwd.  Tokens stay [B*N, D] rows throughout (the
fork transposes to [B, D, N] and back).  The gradients are bitwise reproducible (no float atomics).  Train mode uses the
batch statistics and updates the BatchNorm buffers in place; eval mode reads them and leaves them untouched.  Dropout is
active in train mode with drop > 0: its mask comes from a counter-based generator seeded by an int64 drawn on the device
from the CUDA default generator, and is regenerated in the backward.
compute_dtype: torch.float32 (parity) or torch.bfloat16 (the GEMM operands and activations; LayerNorm and BatchNorm
statistics and every parameter gradient stay float32).  The input and the output are float32.  D a multiple of 8.
"""
import torch
import torch.nn as nn

from . import seq_ops
from ._lib import check, lib
from .ops import MNMAJOR, dt, gemm, ptr, stream
from .seq_ops import convert as _convert, linear_wgrad as _wgrad

PARAMS = ("norm.weight", "norm.bias", "pw_in.weight", "pw_in.bias", "dwconv.weight", "pw_out.weight", "pw_out.bias")


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


def _as(t, dtype):
    """t (contiguous) in the compute dtype: itself, or a converted copy"""
    return t if t.dtype == dtype else _convert(t, _empty(t.shape, dtype, t.device))


def _dropout(x, seed, p):
    y = torch.empty_like(x)
    check(lib.htrvt_sgm_dropout(ptr(x), ptr(y), x.numel(), ptr(seed), p, dt(x.dtype), stream()), "sgm_dropout")
    return y


class _MixerFunction(torch.autograd.Function):
    """(x, parameters) -> y; every step a HIP kernel"""

    @staticmethod
    def forward(ctx, mod, x, p_drop, need, bn_weight, bn_bias, conv_bias, *params):
        P = {n: t.contiguous() for n, t in zip(PARAMS, params)}
        cdt, dev, f32 = mod.compute_dtype, x.device, torch.float32
        B, N, D = x.shape
        R = B * N
        xf = x.contiguous().float().view(R, D)
        xc = _as(xf, cdt)
        w_in, w_out = _as(P["pw_in.weight"], cdt), _as(P["pw_out.weight"], cdt)
        t, mean, rstd = seq_ops.layernorm_fwd(xc, P["norm.weight"], P["norm.bias"], mod.norm.eps)
        u = _empty((R, 2 * D), cdt, dev)
        gemm(t, w_in, u, dtype=cdt, M=R, N=2 * D, K=D, lda=D, ldb=D, ldc=2 * D, bias=P["pw_in.bias"])
        bn = None
        if bn_weight is not None:
            bn = (bn_weight.contiguous(), bn_bias.contiguous(), mod.bn.running_mean, mod.bn.running_var,
                  mod.bn.num_batches_tracked)
        s, saved = seq_ops.conv_mixer_fwd(u, P["dwconv.weight"], B, N, bn=bn, training=mod.training, eps=mod.bn_eps,
                                          momentum=mod.bn_momentum, save=need,
                                          conv_bias=None if conv_bias is None else conv_bias.contiguous())
        o = _empty((R, D), cdt, dev)
        gemm(s, w_out, o, dtype=cdt, M=R, N=D, K=D, lda=D, ldb=D, ldc=D, bias=P["pw_out.bias"])
        seed = None
        if p_drop > 0:
            seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev)     # CUDA default generator, no sync
            o = _dropout(o, seed, p_drop)
        y = _convert(o, _convert(xf, _empty((R, D), f32, dev)), accumulate=True)      # y = x + o, float32
        if need:
            ctx.save_for_backward(xc, mean, rstd, t, u, w_in, w_out, seed, P["norm.weight"], P["dwconv.weight"],
                                  None if bn is None else bn[0], *saved)
            ctx.dims = (B, N, D, float(p_drop), cdt, mod.training, conv_bias is not None)
        else:
            ctx.mark_non_differentiable(y)
        return y.view(B, N, D)

    @staticmethod
    def backward(ctx, dy):
        xc, mean, rstd, t, u, w_in, w_out, seed, ln_w, dw_w, gamma, *saved = ctx.saved_tensors
        B, N, D, p_drop, cdt, training, has_bias = ctx.dims
        R, dev = B * N, xc.device
        dyc = _as(dy.contiguous().float().view(R, D), cdt)
        do = _dropout(dyc, seed, p_drop) if p_drop > 0 else dyc        # the same mask, regenerated from the seed
        s = seq_ops.conv_mixer_act(saved[0], saved[1], saved[2])       # recomputed from c: s is not kept
        dw_out, db_out = _wgrad(do, s, R)
        ds = _empty((R, D), cdt, dev)
        gemm(do, w_out, ds, dtype=cdt, M=R, N=D, K=D, lda=D, ldb=D, ldc=D, b_layout=MNMAJOR)
        du, ddw, dgamma, dbeta, dbias = seq_ops.conv_mixer_bwd(ds, u, dw_w, B, N, saved, gamma=gamma, training=training,
                                                               need_bias=has_bias)
        dw_in, db_in = _wgrad(du, t, R)
        dt_ = _empty((R, D), cdt, dev)
        gemm(du, w_in, dt_, dtype=cdt, M=R, N=D, K=2 * D, lda=2 * D, ldb=D, ldc=D, b_layout=MNMAJOR)
        dln = torch.zeros(2 * D, dtype=torch.float32, device=dev)      # (d weight | d bias) adjacent: one column-sum launch
        dx = seq_ops.layernorm_bwd(dt_, xc, mean, rstd, ln_w, dln[:D], dln[D:], dres=dyc)
        dx = _as(dx, torch.float32).view(B, N, D)
        return (None, dx, None, None, dgamma, dbeta, dbias, dln[:D], dln[D:], dw_in, db_in, ddw, dw_out, db_out)


class ConvLocalMixer1D(nn.Module):
    """Full-width local mixer for [B, N, D]: LN -> 1x1 (2D) -> GLU -> DWConv1d(k) -> BN -> SiLU -> 1x1 -> Dropout -> + x"""

    def __init__(self, dim, kernel_size=7, drop=0.1, use_bn=True, compute_dtype=torch.float32):
        super().__init__()
        if kernel_size % 2 != 1 or not 1 <= kernel_size <= 15:
            raise ValueError(f"ConvLocalMixer1D: kernel_size odd, 1 ... 15, got {kernel_size}")
        if dim % 8:
            raise ValueError(f"ConvLocalMixer1D: dim a multiple of 8, got {dim}")
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"ConvLocalMixer1D: compute_dtype torch.float32 or torch.bfloat16, got {compute_dtype}")
        self.norm = nn.LayerNorm(dim, elementwise_affine=True)
        self.pw_in = nn.Linear(dim, dim * 2, bias=True)
        self.glu = nn.GLU(dim=-1)
        self.dwconv = nn.Conv1d(dim, dim, kernel_size=kernel_size, padding=kernel_size // 2, groups=dim, bias=not use_bn)
        self.bn = nn.BatchNorm1d(dim) if use_bn else nn.Identity()
        self.act = nn.SiLU()
        self.pw_out = nn.Linear(dim, dim, bias=True)
        self.drop = nn.Dropout(drop)
        self.use_bn = use_bn
        self.compute_dtype = compute_dtype

    @property
    def bn_eps(self):
        return self.bn.eps if self.use_bn else 0.0

    @property
    def bn_momentum(self):
        return self.bn.momentum if self.use_bn else 0.0

    def forward(self, x):
        params = [self.get_parameter(n) for n in PARAMS]
        extra = [self.bn.weight, self.bn.bias, None] if self.use_bn else [None, None, self.dwconv.bias]
        if not all(t.is_cuda for t in [x] + params + [t for t in extra if t is not None]):
            raise RuntimeError("ConvLocalMixer1D runs on an MI355X only: move the module and its input to cuda "
                               "(no CPU / eager fallback exists)")
        if x.dim() != 3 or x.shape[2] != self.norm.normalized_shape[0]:
            raise ValueError(f"ConvLocalMixer1D: x [B, N, {self.norm.normalized_shape[0]}] expected, got {tuple(x.shape)}")
        p_drop = float(self.drop.p) if self.training else 0.0
        need = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params + extra if p is not None))
        with torch.cuda.device(x.device):
            return _MixerFunction.apply(self, x, p_drop, need, *extra, *params)
