"""The launch sequences of the attention flavours, norms, the convolutional token mixer, the VAN forks' height reducer
and horizontal mixer, the Swin fork's blocks, the SVTR fork's mixing blocks and the convolutional forks' Conformer /
SqueezeFormer blocks, each written once.

Plain functions over device tensors: no autograd, no Engine state.  They launch on the current stream, allocate with
torch.empty on their input's device, and a forward returns what its backward takes (P or lse, mean / rstd).  Gradient
destinations that the kernels ADD into (dtable, dbias, dgamma / dbeta, dalpha) come from the caller and are not zeroed
here.  Callers: engine.py (the four models), sgm/model/sgm_head.py, mixer.py, van.py, swin.py, svtr.py, conformer.py, and the autograd wrappers of
variants.py.

Self-attention reads qkv [B*N, 3*D] in the qkv Linear's layout [B, N, 3, h, hd]; the score scale is hd^-0.5.

Dropout on the attention probabilities is the keyword `drop=(seed, p)` of the self-attention functions: seed an int64
device tensor of one element, p in (0, 1).  The mask is keep_elem(seed, ((b h + head) N + q) N + k) (csrc/dropout_common.h)
on every route -- regenerated inside the fused kernels, drawn by htrvt_sgm_dropout on P and dP in the unfused one -- and a
backward takes the forward's `drop`.  drop=None is the call without dropout, untouched."""
import collections

import torch

from ._lib import check, lib
from .ops import GATHER_CONV_DGRAD, GATHER_CONV_FWD, GATHER_CONV_WGRAD, MNMAJOR, ConvGeom, colsum, cpad, dt, gemm, ptr, stream


def _f32(x, *shape):
    return torch.empty(*shape, dtype=torch.float32, device=x.device)


def _like(x, *shape):
    return torch.empty(*shape, dtype=x.dtype, device=x.device)


def convert(src, dst, accumulate=False):
    """dst (+)= src between float32 / bfloat16 buffers of equal size"""
    check(lib.htrvt_sgm_convert(ptr(src), dt(src.dtype), ptr(dst), dt(dst.dtype), src.numel(), int(accumulate), stream()),
          "sgm_convert")
    return dst


def linear_wgrad(dy, x, rows, bias=True, split_k=1):
    """a Linear's parameter gradients: dW [N, K] float32 = dy[rows, N]^T x[rows, K]; db [N] = column sums of dy (None
    without `bias`).  split_k > 1: the rows are contracted in that many ranges, each into a float32 slab of its own, added in
    order (reproducible; see wgrad_split_k)"""
    N, K = dy.shape[1], x.shape[1]
    dw = torch.zeros(N, K, dtype=torch.float32, device=dy.device)
    ws = _f32(dy, split_k, N, K) if split_k > 1 else None
    gemm(dy, x, dw, dtype=dy.dtype, M=N, N=K, K=rows, lda=N, ldb=K, ldc=K, a_layout=MNMAJOR, b_layout=MNMAJOR,
         accumulate=True, c_f32=True, split_k=split_k, splitk_ws=ws)
    if not bias:
        return dw, None
    db = torch.zeros(N, dtype=torch.float32, device=dy.device)
    colsum(dy, rows, N, N, db, dti=dt(dy.dtype))
    return dw, db


def dropout(x, seed, p):
    """x * keep / (1 - p) with the counter-based mask of (seed, element index); its backward is the same call on dy"""
    y = torch.empty_like(x)
    check(lib.htrvt_sgm_dropout(ptr(x), ptr(y), x.numel(), ptr(seed), p, dt(x.dtype), stream()), "sgm_dropout")
    return y


def residual_dropout(x, res, rows_per_sample, seeds, p, p_path):
    """res + drop_path(dropout(x)) in one pass over x [rows, D]: element-wise dropout p keyed by (seeds[0], element), the
    whole branch of sample row // rows_per_sample dropped with p_path keyed by (seeds[1], sample).  res=None: without
    the add, which is the backward (dx from dy).  seeds: int64 device tensor of two elements, None when both p are 0."""
    y = torch.empty_like(x)
    check(lib.htrvt_residual_dropout(ptr(x), ptr(res), ptr(y), rows_per_sample, x.numel(), x.shape[-1], ptr(seeds), p, p_path,
                                     dt(x.dtype), stream()), "residual_dropout")
    return y


def drop_add_ln_fwd(x, res, rows_per_sample, seeds, p, p_path, gamma, beta, eps, save=True):
    """residual_dropout and the LayerNorm behind it in one launch (csrc/dropnorm.hip) -> (s, y, mean, rstd):
    s = res + drop_path(dropout(x)) with residual_dropout's masks and keys, y = LayerNorm(s) * gamma + beta with the
    statistics (only under `save`) of s as it is stored, so (s, mean, rstd) is what layernorm_bwd / layernorm_bwd_drop take"""
    rows, D = x.shape
    s, y = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = (_f32(x, rows), _f32(x, rows)) if save else (None, None)
    check(lib.htrvt_drop_add_ln_fwd(ptr(x), ptr(res), ptr(seeds), p, p_path, rows_per_sample, ptr(gamma), ptr(beta), ptr(s), ptr(y),
                                    ptr(mean), ptr(rstd), rows, D, eps, dt(x.dtype), stream()), "drop_add_ln_fwd")
    return s, y, mean, rstd


def mask_tokens_fwd(x, keep, mask_token):
    """y[r] = x[r] where keep[r % keep.numel()] != 0, else mask_token: x [rows, D] float32 / bfloat16, keep float32 with N
    (one mask for the batch) or rows (one flag per row: a [B, N] mask) elements, mask_token float32 [D]"""
    y = torch.empty_like(x)
    check(lib.htrvt_mask_tokens_fwd(ptr(x), ptr(keep), keep.numel(), ptr(mask_token), ptr(y), x.shape[0], x.shape[1],
                                    dt(x.dtype), stream()), "mask_tokens_fwd")
    return y


def mask_tokens_bwd(dy, keep, want_token_grad=True):
    """(dx, d mask_token) of mask_tokens_fwd: dx = dy where kept and 0 where masked; d mask_token [D] float32 = the sum of
    dy over the masked rows through htrvt_colsum's row filter (fixed order, no float atomics), None when not wanted"""
    rows, D = dy.shape
    dx = torch.empty_like(dy)
    check(lib.htrvt_mask_tokens_bwd(ptr(dy), ptr(keep), keep.numel(), ptr(dx), rows, D, dt(dy.dtype), stream()),
          "mask_tokens_bwd")
    dtoken = None
    if want_token_grad:
        dtoken = torch.zeros(D, dtype=torch.float32, device=dy.device)
        colsum(dy, rows, D, D, dtoken, dti=dt(dy.dtype), keep=keep, keep_mod=keep.numel())
    return dx, dtoken


def _heads(qkv, h):
    """(D, hd) of qkv [B*N, 3*D], D = h * hd"""
    D = qkv.shape[1] // 3
    return D, D // h


# ---- affine LayerNorm --------------------------------------------------------------------------------------------------

def layernorm_fwd(x, gamma, beta, eps, save=True):
    """x [rows, D] -> (y, mean, rstd); the statistics only under `save`"""
    rows, D = x.shape
    y = torch.empty_like(x)
    mean, rstd = (_f32(x, rows), _f32(x, rows)) if save else (None, None)
    check(lib.htrvt_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, D, eps, dt(x.dtype),
                                  stream()), "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dres=None):
    """dx (+ dres, the residual branch's gradient); dgamma / dbeta += the ordered column sum of the per-block partials"""
    rows, D = x.shape
    nblk = lib.htrvt_layernorm_bwd_blocks(rows)
    partial = _f32(x, nblk, 2, D)
    dx = torch.empty_like(x)
    check(lib.htrvt_layernorm_bwd(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(dx), ptr(partial),
                                  rows, D, dt(x.dtype), stream()), "layernorm_bwd")
    _ln_param_grads(partial, nblk, D, dgamma, dbeta)
    return dx


def _ln_param_grads(partial, nblk, D, dgamma, dbeta):
    if dbeta.data_ptr() == dgamma.data_ptr() + 4 * D:   # weight and bias adjacent in one float32 buffer: one launch
        colsum(partial, nblk, 2 * D, 2 * D, dgamma, dti=0)
    else:
        colsum(partial, nblk, D, 2 * D, dgamma, dti=0)
        colsum(partial.data_ptr() + 4 * D, nblk, D, 2 * D, dbeta, dti=0)


def layernorm_bwd_drop(dy, s, mean, rstd, gamma, dgamma, dbeta, rows_per_sample, seeds, p, p_path, dres=None):
    """layernorm_bwd at the s of drop_add_ln_fwd and the residual_dropout backward behind it in one launch -> (ds, dxb):
    ds the residual stream's gradient (+ dres), dxb = ds * keepE / (1 - p) * keepS / (1 - p_path) the branch's"""
    rows, D = s.shape
    nblk = lib.htrvt_layernorm_bwd_blocks(rows)
    partial = _f32(s, nblk, 2, D)
    ds, dxb = torch.empty_like(s), torch.empty_like(s)
    check(lib.htrvt_layernorm_bwd_drop(ptr(dy), ptr(s), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(seeds), p, p_path,
                                       rows_per_sample, ptr(ds), ptr(dxb), ptr(partial), rows, D, dt(s.dtype), stream()),
          "layernorm_bwd_drop")
    _ln_param_grads(partial, nblk, D, dgamma, dbeta)
    return ds, dxb


# ---- self-attention, fused (csrc/attention.hip): scores / probabilities stay on chip -----------------------------------

def _plain_only(bias, drop):
    if drop is not None and bias is not None:
        raise ValueError("fused attention: dropout with a dense score bias is not served (the table kernels or the unfused route)")


def attention_fwd(qkv, B, N, h, bias=None, save=True, drop=None):
    """(out [B*N, D], lse [B*h, N] or None); bias: None or dense float32 [h, N, N]; drop: (seed, p), plain scores only"""
    D, hd = _heads(qkv, h)
    out = _like(qkv, B * N, D)
    lse = _f32(qkv, B * h, N) if save else None
    _plain_only(bias, drop)
    if drop is not None:
        check(lib.htrvt_attn_dropout_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, h, hd, hd ** -0.5, ptr(drop[0]), drop[1],
                                         dt(qkv.dtype), stream()), "attn_dropout_fwd")
        return out, lse
    check(lib.htrvt_attn_fwd(ptr(qkv), ptr(bias), ptr(out), ptr(lse), B, N, h, hd, hd ** -0.5, dt(qkv.dtype), stream()),
          "attn_fwd")
    return out, lse


def attention_bwd(qkv, out, dout, lse, B, N, h, bias=None, dbias=None, drop=None):
    """dqkv by the recomputing backward; dbias (float32 [h, N, N]) += d(score) summed over the batch"""
    hd = _heads(qkv, h)[1]
    dqkv = torch.empty_like(qkv)
    delta = _f32(qkv, B * h, N)
    _plain_only(bias, drop)
    if drop is not None:
        check(lib.htrvt_attn_dropout_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), B, N, h, hd,
                                         hd ** -0.5, ptr(drop[0]), drop[1], dt(qkv.dtype), stream()), "attn_dropout_bwd")
        return dqkv
    check(lib.htrvt_attn_bwd(ptr(qkv), ptr(bias), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), ptr(dbias), B, N, h,
                             hd, hd ** -0.5, dt(qkv.dtype), stream()), "attn_bwd")
    return dqkv


# ---- self-attention as batched GEMMs + row softmax: float32, and shapes the fused kernels do not serve -----------------

def attention_unfused_fwd(qkv, B, N, h, bias=None, drop=None):
    """S = scale q k^T, P = softmax(S + bias), out = P v -> (out, P [B*h, N, N], kept for the backward).  drop: out =
    dropout(P) v; the P returned is the undropped one (the backward redraws the mask)"""
    D, hd = _heads(qkv, h)
    out = _like(qkv, B * N, D)
    S = _f32(qkv, B * h, N, N)
    gemm(qkv, qkv, S, dtype=qkv.dtype, M=N, N=N, K=hd, lda=3 * D, ldb=3 * D, ldc=N, batch=B * h, batch_inner=h,
         sA=(N * 3 * D, hd), sB=(N * 3 * D, hd), sC=(h * N * N, N * N), b_off=D, alpha=hd ** -0.5, c_f32=True)
    P = _like(qkv, B * h, N, N)
    check(lib.htrvt_softmax_rows(ptr(S), ptr(P), B * h * N, N, dt(qkv.dtype), ptr(bias), h * N if bias is not None else 0,
                                 stream()), "softmax_rows")
    del S
    Pv = P if drop is None else dropout(P, *drop)
    gemm(Pv, qkv, out, dtype=qkv.dtype, M=N, N=hd, K=N, lda=N, ldb=3 * D, ldc=D, b_layout=MNMAJOR, batch=B * h,
         batch_inner=h, sA=(h * N * N, N * N), sB=(N * 3 * D, hd), sC=(N * D, hd), b_off=2 * D)
    return out, P


def attention_unfused_bwd(qkv, P, dout, B, N, h, dbias=None, drop=None):
    """dqkv over the saved P.  Without dbias the score scale goes into the softmax backward; with dbias (float32
    [h, N, N], += d(score) summed over the batch) dS stays unscaled and the dQ / dK GEMMs carry the scale."""
    D, hd = _heads(qkv, h)
    scale = hd ** -0.5
    dqkv = torch.empty_like(qkv)
    bstr = dict(batch=B * h, batch_inner=h)
    # dV = P^T dO (dropout: the P that multiplied V)
    gemm(P if drop is None else dropout(P, *drop), dout, dqkv, dtype=qkv.dtype, M=N, N=hd, K=N, lda=N, ldb=D, ldc=3 * D, a_layout=MNMAJOR, b_layout=MNMAJOR,
         sA=(h * N * N, N * N), sB=(N * D, hd), sC=(N * 3 * D, hd), c_off=2 * D, **bstr)
    # dP = dO V^T
    dP = _f32(qkv, B * h, N, N)
    gemm(dout, qkv, dP, dtype=qkv.dtype, M=N, N=N, K=hd, lda=D, ldb=3 * D, ldc=N, sA=(N * D, hd), sB=(N * 3 * D, hd),
         sC=(h * N * N, N * N), b_off=2 * D, c_f32=True, **bstr)
    if drop is not None:
        dP = dropout(dP, *drop)
    dS = _like(qkv, B * h, N, N)
    s_in, s_out = (scale, 1.0) if dbias is None else (1.0, scale)
    check(lib.htrvt_softmax_bwd_rows(ptr(P), ptr(dP), ptr(dS), B * h * N, N, s_in, dt(qkv.dtype), stream()),
          "softmax_bwd_rows")
    del dP
    if dbias is not None:
        colsum(dS, B, h * N * N, h * N * N, dbias, dti=dt(qkv.dtype))
    # dQ = dS K ; dK = dS^T Q
    gemm(dS, qkv, dqkv, dtype=qkv.dtype, M=N, N=hd, K=N, lda=N, ldb=3 * D, ldc=3 * D, b_layout=MNMAJOR, alpha=s_out,
         sA=(h * N * N, N * N), sB=(N * 3 * D, hd), sC=(N * 3 * D, hd), b_off=D, c_off=0, **bstr)
    gemm(dS, qkv, dqkv, dtype=qkv.dtype, M=N, N=hd, K=N, lda=N, ldb=3 * D, ldc=3 * D, a_layout=MNMAJOR, alpha=s_out,
         b_layout=MNMAJOR, sA=(h * N * N, N * N), sB=(N * 3 * D, hd), sC=(N * 3 * D, hd), b_off=0, c_off=D, **bstr)
    return dqkv


# ---- window fork: relative-position table [(2P-1), h] float32, 1-D (shifted) windows -----------------------------------

def relpos_workspace_floats(B, N, h, num_patches, window=0, shift=0):
    n = lib.htrvt_attn_relpos_bwd_workspace_floats(B, N, h, num_patches, window, shift)
    if n < 0:
        raise ValueError(f"relative-position attention: {lib.htrvt_last_error().decode()}")
    return n


def relpos_attention_fwd(qkv, table, B, N, h, num_patches, window, shift, save=True, drop=None):
    """table-driven fused kernels (csrc/attn_relpos.hip, bfloat16): (out, lse or None)"""
    D, hd = _heads(qkv, h)
    out = _like(qkv, B * N, D)
    lse = _f32(qkv, B * h, N) if save else None
    if drop is not None:
        check(lib.htrvt_attn_relpos_dropout_fwd(ptr(qkv), ptr(table), ptr(out), ptr(lse), B, N, h, hd, hd ** -0.5, num_patches,
                                                window, shift, ptr(drop[0]), drop[1], dt(qkv.dtype), stream()),
              "attn_relpos_dropout_fwd")
        return out, lse
    check(lib.htrvt_attn_relpos_fwd(ptr(qkv), ptr(table), ptr(out), ptr(lse), B, N, h, hd, hd ** -0.5, num_patches, window,
                                    shift, dt(qkv.dtype), stream()), "attn_relpos_fwd")
    return out, lse


def relpos_attention_bwd(qkv, table, out, dout, lse, B, N, h, num_patches, window, shift, dtable=None, drop=None):
    """dqkv; dtable (float32, the table's shape) += the table gradient, None: no table gradient and no workspace"""
    hd = _heads(qkv, h)[1]
    dqkv = torch.empty_like(qkv)
    delta = _f32(qkv, B * h, N)
    work = None if dtable is None else _f32(qkv, relpos_workspace_floats(B, N, h, num_patches, window, shift))
    if drop is not None:
        check(lib.htrvt_attn_relpos_dropout_bwd(ptr(qkv), ptr(table), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv),
                                                ptr(dtable), ptr(work), B, N, h, hd, hd ** -0.5, num_patches, window, shift,
                                                ptr(drop[0]), drop[1], dt(qkv.dtype), stream()), "attn_relpos_dropout_bwd")
        return dqkv
    check(lib.htrvt_attn_relpos_bwd(ptr(qkv), ptr(table), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), ptr(dtable),
                                    ptr(work), B, N, h, hd, hd ** -0.5, num_patches, window, shift, dt(qkv.dtype), stream()),
          "attn_relpos_bwd")
    return dqkv


def relpos_bias_fwd(table, N, num_patches, window, shift, ld):
    """dense float32 bias [h, ld, ld] for the unfused route: table entries inside a window, -1e30 outside and at
    columns >= N (csrc/variants.hip)"""
    h = table.shape[1]
    bias = _f32(table, h, ld, ld)
    check(lib.htrvt_relpos_bias_fwd(ptr(table), ptr(bias), N, num_patches, window, shift, h, ld, stream()), "relpos_bias_fwd")
    return bias


def relpos_bias_bwd(dbias, N, num_patches, window, shift):
    """dense d(bias) [h, ld, ld] -> the table's gradient [(2P-1), h] (written, not added: a per-entry gather-sum)"""
    h, ld = dbias.shape[0], dbias.shape[-1]
    dtable = _f32(dbias, 2 * num_patches - 1, h)
    check(lib.htrvt_relpos_bias_bwd(ptr(dbias), ptr(dtable), N, num_patches, window, shift, h, ld, stream()), "relpos_bias_bwd")
    return dtable


# ---- SGM head: single-head cross-attention softmax(Q K^T / sqrt(D)) K, K = V -------------------------------------------

def cross_attention_fwd(Q, KV):
    """Q [B, L, D], KV [B, N, D] -> (out [B, L, D], P [B, L, N])"""
    B, L, D = Q.shape
    N = KV.shape[1]
    S = _f32(Q, B, L, N)
    gemm(Q, KV, S, dtype=Q.dtype, M=L, N=N, K=D, lda=D, ldb=D, ldc=N, batch=B, sA=(L * D, 0), sB=(N * D, 0), sC=(L * N, 0),
         alpha=D ** -0.5, c_f32=True)
    P = _like(Q, B, L, N)
    check(lib.htrvt_softmax_rows(ptr(S), ptr(P), B * L, N, dt(Q.dtype), None, 0, stream()), "softmax_rows")
    out = _like(Q, B, L, D)
    gemm(P, KV, out, dtype=Q.dtype, M=L, N=D, K=N, lda=N, ldb=D, ldc=D, b_layout=MNMAJOR, batch=B, sA=(L * N, 0),
         sB=(N * D, 0), sC=(L * D, 0))
    return out, P


def cross_attention_bwd(Q, KV, P, dout):
    """(dQ, dKV); dKV sums the paths through V (P^T dO) and through K (dS^T Q)"""
    B, L, D = Q.shape
    N = KV.shape[1]
    dtype = Q.dtype
    bb = dict(batch=B)
    dP = _f32(Q, B, L, N)
    gemm(dout, KV, dP, dtype=dtype, M=L, N=N, K=D, lda=D, ldb=D, ldc=N, sA=(L * D, 0), sB=(N * D, 0), sC=(L * N, 0),
         c_f32=True, **bb)                                                        # dP = dO V^T
    dS = _like(Q, B, L, N)
    check(lib.htrvt_softmax_bwd_rows(ptr(P), ptr(dP), ptr(dS), B * L, N, D ** -0.5, dt(dtype), stream()), "softmax_bwd_rows")
    dQ = torch.empty_like(Q)
    gemm(dS, KV, dQ, dtype=dtype, M=L, N=D, K=N, lda=N, ldb=D, ldc=D, b_layout=MNMAJOR, sA=(L * N, 0), sB=(N * D, 0),
         sC=(L * D, 0), **bb)                                                     # dQ = dS K
    dKV = torch.empty_like(KV)
    gemm(P, dout, dKV, dtype=dtype, M=N, N=D, K=L, lda=N, ldb=D, ldc=D, a_layout=MNMAJOR, b_layout=MNMAJOR,
         sA=(L * N, 0), sB=(L * D, 0), sC=(N * D, 0), **bb)                       # through V: P^T dO
    gemm(dS, Q, dKV, dtype=dtype, M=N, N=D, K=L, lda=N, ldb=D, ldc=D, a_layout=MNMAJOR, b_layout=MNMAJOR,
         sA=(L * N, 0), sB=(L * D, 0), sC=(N * D, 0), residual=dKV, **bb)         # + through K: dS^T Q
    return dQ, dKV


# ---- LGP fork (csrc/lgp.hip): window-12 attention, pool + LayerNorm, up-sample * sigmoid(alpha) -------------------------

def local_attention_fwd(qkv, qkv_bias, B, N, h, window, shift=0):
    """attention inside windows of `window` tokens; the padding slots of a ragged last window are rows equal to the qkv
    Linear's float32 bias.  shift (0 ... window - 1): the windows are those of the tokens rolled by `shift`"""
    D, hd = _heads(qkv, h)
    out = _like(qkv, B * N, D)
    check(lib.htrvt_attn_local_shift_fwd(ptr(qkv), ptr(qkv_bias), ptr(out), B, N, h, hd, window, shift, hd ** -0.5,
                                         dt(qkv.dtype), stream()), "attn_local_shift_fwd")
    return out


def local_attention_bwd(qkv, qkv_bias, dout, B, N, h, window, shift=0):
    """(dqkv, dpad float32 [B, 2*D]: per image the gradient of the padding rows' k / v, meaningful where N % window; its
    column sum belongs to the k / v thirds of the bias gradient)"""
    D, hd = _heads(qkv, h)
    dqkv = torch.empty_like(qkv)
    dpad = _f32(qkv, B, 2 * D)
    check(lib.htrvt_attn_local_shift_bwd(ptr(qkv), ptr(qkv_bias), ptr(dout), ptr(dqkv), ptr(dpad), B, N, h, hd, window, shift,
                                         hd ** -0.5, dt(qkv.dtype), stream()), "attn_local_shift_bwd")
    return dqkv, dpad


def pool_norm_fwd(x, B, N, G, eps):
    """average pooling of x [B*N, D] to G tokens per image + LayerNorm without affine -> (z [B*G, D], mean, rstd)"""
    D = x.shape[1]
    z = _like(x, B * G, D)
    mean, rstd = _f32(x, B * G), _f32(x, B * G)
    check(lib.htrvt_lgp_pool_norm_fwd(ptr(x), ptr(z), ptr(mean), ptr(rstd), B, N, G, D, eps, dt(x.dtype), stream()),
          "lgp_pool_norm_fwd")
    return z, mean, rstd


def pool_norm_bwd(dz, z, rstd, B, N, G, dx=None):
    """the gradient of x: a new tensor, or added into `dx` [B*N, D] where one is given"""
    D = z.shape[1]
    add = dx is not None
    if not add:
        dx = _like(z, B * N, D)
    ws = _f32(z, 2 * B * G)
    check(lib.htrvt_lgp_pool_norm_bwd(ptr(dz), ptr(z), ptr(rstd), ptr(ws), ptr(dx), B, N, G, D, int(add), dt(z.dtype), stream()),
          "lgp_pool_norm_bwd")
    return dx


def upsample_fwd(y, logit_alpha, out, B, N, G):
    """out [B*N, D] (may be a column block such as cat[:, D:]) = y [B*G, D] linearly interpolated to N tokens per image,
    times sigmoid(logit_alpha)"""
    D = y.shape[1]
    assert out.shape[1] == D and out.stride(1) == 1
    check(lib.htrvt_lgp_upsample_fwd(ptr(y), ptr(logit_alpha), ptr(out), out.stride(0), B, N, G, D, dt(y.dtype), stream()),
          "lgp_upsample_fwd")
    return out


def upsample_bwd(dout, y, logit_alpha, dalpha, B, N, G):
    """dy [B*G, D]; dalpha (0-dim float32) += d logit_alpha.  dout may be a column block, as in upsample_fwd."""
    D = y.shape[1]
    assert dout.shape[1] == D and dout.stride(1) == 1
    dy = torch.empty_like(y)
    ws = _f32(y, lib.htrvt_lgp_upsample_bwd_workspace_floats(B, G))
    check(lib.htrvt_lgp_upsample_bwd(ptr(dout), dout.stride(0), ptr(y), ptr(logit_alpha), ptr(dy), ptr(dalpha), ptr(ws), B, N, G,
                                     D, dt(y.dtype), stream()), "lgp_upsample_bwd")
    return dy


# ---- macaron forks (csrc/mixer.hip): GLU -> depthwise token conv -> BatchNorm1d -> SiLU between the mixer's Linear layers

def conv_mixer_fwd(u, weight, B, N, bn=None, training=False, eps=1e-5, momentum=0.1, conv_bias=None, save=True):
    """u [B*N, 2*D] (pw_in's output), weight float32 [D, 1, k] -> (s [B*N, D], saved).  bn: None (use_bn=False: z = c +
    conv_bias) or (gamma, beta, running_mean, running_var, num_batches_tracked); in training mode the batch statistics
    are used and the three buffers updated in place, else the running ones.  saved = (c, scale, shift, mean, rstd) for
    conv_mixer_bwd: c [B*N, D] is the convolution's output (None without `save` outside training), the rest float32 [D]
    or None."""
    D, k, dti, st = u.shape[1] // 2, weight.shape[-1], dt(u.dtype), stream()
    s = _like(u, B * N, D)
    if bn is None:
        c = _like(u, B * N, D) if save else None
        check(lib.htrvt_mixer_fwd_eval(ptr(u), ptr(weight), None, ptr(conv_bias), ptr(c), ptr(s), B, N, D, k, dti, st),
              "mixer_fwd_eval")
        return s, (c, None, conv_bias, None, None)
    gamma, beta, rmean, rvar, nbt = bn
    scale, shift, rstd = _f32(u, D), _f32(u, D), _f32(u, D)
    if not training:
        c = _like(u, B * N, D) if save else None
        check(lib.htrvt_bn_eval_coeffs(ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), eps, ptr(scale), ptr(shift), ptr(rstd),
                                       D, st), "bn_eval_coeffs")
        check(lib.htrvt_mixer_fwd_eval(ptr(u), ptr(weight), ptr(scale), ptr(shift), ptr(c), ptr(s), B, N, D, k, dti, st),
              "mixer_fwd_eval")
        return s, (c, scale, shift, rmean.clone() if save else None, rstd)
    nws = lib.htrvt_mixer_fwd_workspace_floats(B, N, D, dti)
    if nws < 0:
        check(-1, "mixer_fwd_train")
    c, partial, mean = _like(u, B * N, D), _f32(u, nws), _f32(u, D)
    check(lib.htrvt_mixer_fwd_train(ptr(u), ptr(weight), ptr(c), ptr(partial), B, N, D, k, dti, st), "mixer_fwd_train")
    check(lib.htrvt_bn_finalize(ptr(partial), lib.htrvt_mixer_rows(B, N, D, dti), D, float(B * N), ptr(gamma), ptr(beta), eps,
                                momentum, ptr(rmean), ptr(rvar), ptr(nbt), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), st),
          "bn_finalize")
    conv_mixer_act(c, scale, shift, s)
    return s, (c, scale, shift, mean, rstd)


def conv_mixer_act(c, scale, shift, s=None):
    """s = silu(c * scale + shift): the train forward's second pass, and the backward's way to s without keeping it"""
    s = torch.empty_like(c) if s is None else s
    check(lib.htrvt_mixer_bn_silu(ptr(c), ptr(scale), ptr(shift), ptr(s), c.shape[0], c.shape[1], dt(c.dtype), stream()),
          "mixer_bn_silu")
    return s


def conv_mixer_bwd(ds, u, weight, B, N, saved, gamma=None, training=False, need_bias=False):
    """ds [B*N, D] -> (du [B*N, 2*D], dweight [D, 1, k], dgamma, dbeta, dbias), float32 parameter gradients; dgamma / dbeta
    are None without BatchNorm (gamma None), dbias is None unless need_bias"""
    c, scale, shift, mean, rstd = saved
    D, k, dti, st = u.shape[1] // 2, weight.shape[-1], dt(u.dtype), stream()
    dgamma = dbeta = coef = None
    if gamma is not None:
        nred = lib.htrvt_mixer_reduce_rows(B * N, D, dti)
        partial, coef = _f32(u, nred, 2, D), _f32(u, 3, D)
        check(lib.htrvt_mixer_bwd_reduce(ptr(ds), ptr(c), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(partial), B * N, D,
                                         dti, st), "mixer_bwd_reduce")
        dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
        check(lib.htrvt_bn_bwd_finalize(ptr(partial), nred, D, float(B * N) if training else 0.0, ptr(gamma), ptr(mean),
                                        ptr(rstd), ptr(dgamma), ptr(dbeta), ptr(coef), st), "bn_bwd_finalize")
    rows = lib.htrvt_mixer_rows(B, N, D, dti)
    if rows < 0:
        check(-1, "mixer_bwd")
    pw = _f32(u, rows, D * k)
    pb = _f32(u, rows, D) if need_bias else None
    du = torch.empty_like(u)
    check(lib.htrvt_mixer_bwd(ptr(u), ptr(c), ptr(ds), ptr(weight), ptr(scale), ptr(shift), ptr(coef), ptr(du), ptr(pw), ptr(pb),
                              B, N, D, k, dti, st), "mixer_bwd")
    dweight = torch.zeros_like(weight)
    colsum(pw, rows, D * k, D * k, dweight, dti=0)
    dbias = None
    if need_bias:
        dbias = torch.zeros(D, dtype=torch.float32, device=u.device)
        colsum(pb, rows, D, D, dbias, dti=0)
    return du, dweight, dgamma, dbeta, dbias


# ---- VAN forks (csrc/van.hip): VANBlock and HorizontalMixer of model_sgm_mms_attach_van/model/HTR_VT.py on NHWC ----------
# Activations are x [B, H, W, C] (contiguous, float32 or bfloat16) and, for the 1x1 convolutions and the BatchNorm passes,
# the same memory as rows [B*H*W, C].  Depthwise weights are the Conv2d parameters [C, 1, kh, kw] float32; the 1x1 weights
# come as [C, C] in the activations' dtype.  A BatchNorm is bn = (gamma, beta, running_mean, running_var,
# num_batches_tracked), all as stored; in training mode the three buffers are updated in place.

def dwconv_fwd(x, weight, dilation=1):
    """depthwise Conv2d(C, C, (kh, kw), padding = (k // 2) * dilation, dilation, groups = C, bias = False) of x NHWC"""
    B, H, W, C = x.shape
    kh, kw = weight.shape[-2:]
    y = torch.empty_like(x)
    check(lib.htrvt_van_dw_fwd(ptr(x), ptr(weight), ptr(y), B, H, W, C, kh, kw, dilation, dt(x.dtype), stream()), "van_dw_fwd")
    return y


def dwconv_bwd(dy, x, weight, dilation=1, add=None):
    """(dx (+ add, a gradient that reaches x by another path), dweight float32 of weight's shape)"""
    B, H, W, C = x.shape
    kh, kw = weight.shape[-2:]
    geo = (B, H, W, C, kh, kw, dilation, dt(x.dtype))
    rows = lib.htrvt_van_dw_rows(*geo)
    if rows < 0:
        check(-1, "van_dw_rows")
    dx = torch.empty_like(x)
    check(lib.htrvt_van_dw_bwd_input(ptr(dy), ptr(weight), ptr(add), ptr(dx), *geo, stream()), "van_dw_bwd_input")
    partial = _f32(x, rows, C * kh * kw)
    check(lib.htrvt_van_dw_bwd_weight(ptr(x), ptr(dy), ptr(partial), *geo, stream()), "van_dw_bwd_weight")
    dweight = torch.zeros_like(weight)
    colsum(partial, rows, C * kh * kw, C * kh * kw, dweight, dti=0)
    return dx, dweight


def bn_coeffs(x, bn, training, eps, momentum):
    """(scale, shift, mean, rstd) float32 [C] of BatchNorm2d over x [rows, C]: the batch statistics of x as stored (and the
    running buffers updated) in training mode, else the running ones"""
    rows, C = x.shape
    gamma, beta, rmean, rvar, nbt = bn
    scale, shift, mean, rstd = _f32(x, C), _f32(x, C), _f32(x, C), _f32(x, C)
    if not training:
        check(lib.htrvt_bn_eval_coeffs(ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), eps, ptr(scale), ptr(shift), ptr(rstd), C,
                                       stream()), "bn_eval_coeffs")
        return scale, shift, rmean.clone(), rstd
    if rows < 2:
        raise ValueError("BatchNorm in training mode needs more than one value per channel")
    Q = lib.htrvt_van_moments_rows(rows, C, dt(x.dtype))
    if Q < 0:
        check(-1, "van_moments_rows")
    partial = _f32(x, Q, 2, C)
    check(lib.htrvt_van_moments(ptr(x), ptr(partial), rows, C, dt(x.dtype), stream()), "van_moments")
    check(lib.htrvt_bn_finalize(ptr(partial), Q, C, float(rows), ptr(gamma), ptr(beta), eps, momentum, ptr(rmean), ptr(rvar),
                                ptr(nbt), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), stream()), "bn_finalize")
    return scale, shift, mean, rstd


def bn_bwd(dz, x, gamma, mean, rstd, training):
    """BatchNorm backward over [rows, C] on the htrvt_bn_bwd_* passes: dz the gradient of the output, x the input ->
    (dx, dgamma, dbeta); eval mode: the statistics are constants"""
    rows, C = x.shape
    dti, st = dt(x.dtype), stream()
    nblk = lib.htrvt_bn_bwd_blocks(rows)
    partial, coef = _f32(x, nblk, 2, C), _f32(x, 3, C)
    check(lib.htrvt_bn_bwd_reduce(ptr(dz), None, ptr(x), ptr(mean), ptr(rstd), ptr(partial), rows, C, dti, st), "bn_bwd_reduce")
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
    check(lib.htrvt_bn_bwd_finalize(ptr(partial), nblk, C, float(rows) if training else 0.0, ptr(gamma), ptr(mean), ptr(rstd),
                                    ptr(dgamma), ptr(dbeta), ptr(coef), st), "bn_bwd_finalize")
    dx = torch.empty_like(x)
    check(lib.htrvt_bn_bwd_apply(ptr(dz), None, ptr(x), ptr(coef), ptr(dx), None, rows, C, dti, st), "bn_bwd_apply")
    return dx, dgamma, dbeta


def wgrad_split_k(rows, N, K):
    """split-K factor of a [N, K] weight gradient over `rows` rows: a power of two, ranges of at least 2048 rows, no more
    (range, 256 x 192 tile) pairs than the 256 CUs -- a 768 x 768 gradient is 12 tiles, which alone would leave 244 CUs idle
    over the 65 536 rows of the forks' map"""
    tiles = ((N + 255) // 256) * ((K + 191) // 192)
    sk = 1
    while 2 * sk <= min(rows // 2048, 256 // tiles):
        sk *= 2
    return sk


def _pw_wgrad(dy, x, bias=True):
    """(dW, db) of a 1x1 convolution on rows"""
    rows = dy.shape[0]
    return linear_wgrad(dy, x, rows, bias=bias, split_k=wgrad_split_k(rows, dy.shape[1], x.shape[1]))


def _pw(x, w, **kw):
    """1x1 convolution of x [rows, C] with w [Cout, C]"""
    rows, C = x.shape
    y = _like(x, rows, w.shape[0])
    gemm(x, w, y, dtype=x.dtype, M=rows, N=w.shape[0], K=C, lda=C, ldb=C, ldc=w.shape[0], **kw)
    return y


def _pw_dgrad(dy, w, **kw):
    rows, N = dy.shape
    dx = _like(dy, rows, w.shape[1])
    gemm(dy, w, dx, dtype=dy.dtype, M=rows, N=w.shape[1], K=N, lda=N, ldb=w.shape[1], ldc=w.shape[1], b_layout=MNMAJOR, **kw)
    return dx


def lka_fwd(a, dw_w, dwd_w, pw_w, bn, training, eps, momentum):
    """LargeKernelAttention on a [B, H, W, C]: a * bn(pw(dwd(dw(a)))), dw 5x5, dwd 7x7 dilation 3 -> (g, saved)"""
    C = a.shape[-1]
    d1 = dwconv_fwd(a, dw_w, 1)
    d2 = dwconv_fwd(d1, dwd_w, 3)
    p = _pw(d2.view(-1, C), pw_w)
    scale, shift, mean, rstd = bn_coeffs(p, bn, training, eps, momentum)
    g = torch.empty_like(p)
    check(lib.htrvt_van_gate_fwd(ptr(a), ptr(p), ptr(scale), ptr(shift), ptr(g), p.shape[0], C, dt(a.dtype), stream()),
          "van_gate_fwd")
    return g, (d1, d2, p, scale, shift, mean, rstd)


def lka_bwd(dg, a, dw_w, dwd_w, pw_w, gamma, saved, training):
    """dg [rows, C] -> (da [B, H, W, C], {parameter gradients, float32})"""
    d1, d2, p, scale, shift, mean, rstd = saved
    rows, C = p.shape
    da, dz = torch.empty_like(p), torch.empty_like(p)
    check(lib.htrvt_van_gate_bwd(ptr(dg), ptr(a), ptr(p), ptr(scale), ptr(shift), ptr(da), ptr(dz), rows, C, dt(a.dtype),
                                 stream()), "van_gate_bwd")
    dp, dgamma, dbeta = bn_bwd(dz, p, gamma, mean, rstd, training)
    dpw = _pw_wgrad(dp, d2.view(rows, C), bias=False)[0]
    dd2 = _pw_dgrad(dp, pw_w).view(a.shape)
    dd1, ddwd = dwconv_bwd(dd2, d1, dwd_w, 3)
    da, ddw = dwconv_bwd(dd1, a, dw_w, 1, add=da.view(a.shape))
    return da, {"dw.weight": ddw, "dwd.weight": ddwd, "pw.weight": dpw, "bn.weight": dgamma, "bn.bias": dbeta}


def van_block_fwd(x, P, lka_bn, norm_bn, training, eps, momentum):
    """VANBlock on x [B, H, W, C]: x + norm(proj2(lka(gelu(proj1(x))))).  P: the block's parameters by the fork's names,
    the four 1x1 weights as [C, C] in x's dtype -> (y, saved)"""
    C = x.shape[-1]
    xr = x.view(-1, C)
    pre = torch.empty_like(xr)
    a = _pw(xr, P["proj1.weight"], bias=P["proj1.bias"], act=1, preact=pre).view(x.shape)
    g, lka_saved = lka_fwd(a, P["lka.dw.weight"], P["lka.dwd.weight"], P["lka.pw.weight"], lka_bn, training, eps[0], momentum[0])
    q = _pw(g, P["proj2.weight"], bias=P["proj2.bias"])
    scale, shift, mean, rstd = bn_coeffs(q, norm_bn, training, eps[1], momentum[1])
    y = torch.empty_like(x)
    check(lib.htrvt_bn_apply(ptr(q), ptr(scale), ptr(shift), ptr(x), None, None, ptr(y), q.shape[0], C, 0, dt(x.dtype),
                             stream()), "bn_apply")
    return y, (pre, a, g, q, mean, rstd) + lka_saved


def van_block_bwd(dy, x, P, saved, training):
    """dy [B, H, W, C] -> (dx, {parameter gradients by the fork's names, float32})"""
    pre, a, g, q, mean, rstd, *lka_saved = saved
    rows, C = q.shape
    dyr = dy.view(rows, C)
    dq, dgamma, dbeta = bn_bwd(dyr, q, P["norm.weight"], mean, rstd, training)
    dw2, db2 = _pw_wgrad(dq, g)
    dg = _pw_dgrad(dq, P["proj2.weight"])
    da, grads = lka_bwd(dg, a, P["lka.dw.weight"], P["lka.dwd.weight"], P["lka.pw.weight"], P["lka.bn.weight"], lka_saved,
                        training)
    dpre = torch.empty_like(pre)
    check(lib.htrvt_van_bn_res_gelu_bwd(ptr(da), ptr(pre), None, None, None, ptr(dpre), rows, C, dt(x.dtype), stream()),
          "van_bn_res_gelu_bwd")
    dw1, db1 = _pw_wgrad(dpre, x.view(rows, C))
    dx = _pw_dgrad(dpre, P["proj1.weight"], residual=dyr).view(x.shape)
    grads = {"lka." + k: v for k, v in grads.items()}
    grads.update({"proj1.weight": dw1, "proj1.bias": db1, "proj2.weight": dw2, "proj2.bias": db2, "norm.weight": dgamma,
                  "norm.bias": dbeta})
    return dx, grads


def hmixer_fwd(x, dw_w, pw_w, bn, training, eps, momentum):
    """HorizontalMixer on x [B, 1, W, C]: gelu(x + bn(pw(dw(x)))), dw 1 x k -> (y, saved)"""
    C = x.shape[-1]
    d = dwconv_fwd(x, dw_w, 1)
    p = _pw(d.view(-1, C), pw_w)
    scale, shift, mean, rstd = bn_coeffs(p, bn, training, eps, momentum)
    y = torch.empty_like(x)
    check(lib.htrvt_van_bn_res_gelu_fwd(ptr(p), ptr(scale), ptr(shift), ptr(x), ptr(y), p.shape[0], C, dt(x.dtype), stream()),
          "van_bn_res_gelu_fwd")
    return y, (d, p, scale, shift, mean, rstd)


def hmixer_bwd(dy, x, dw_w, pw_w, gamma, saved, training):
    """dy [B, 1, W, C] -> (dx, {parameter gradients, float32})"""
    d, p, scale, shift, mean, rstd = saved
    rows, C = p.shape
    dt_ = torch.empty_like(p)
    check(lib.htrvt_van_bn_res_gelu_bwd(ptr(dy), ptr(p), ptr(scale), ptr(shift), ptr(x), ptr(dt_), rows, C, dt(x.dtype),
                                        stream()), "van_bn_res_gelu_bwd")
    dp, dgamma, dbeta = bn_bwd(dt_, p, gamma, mean, rstd, training)
    dpw = _pw_wgrad(dp, d.view(rows, C), bias=False)[0]
    dd = _pw_dgrad(dp, pw_w).view(x.shape)
    dx, ddw = dwconv_bwd(dd, x, dw_w, 1, add=dt_.view(x.shape))
    return dx, {"dw.weight": ddw, "pw.weight": dpw, "bn.weight": dgamma, "bn.bias": dbeta}


def height_pool_fwd(x):
    """x [B, H, W, C] -> the mean over H, [B, W, C]"""
    B, H, W, C = x.shape
    y = _like(x, B, W, C)
    check(lib.htrvt_van_hpool_fwd(ptr(x), ptr(y), B, H, W, C, dt(x.dtype), stream()), "van_hpool_fwd")
    return y


def height_pool_bwd(d, H):
    """d [B, W, C] -> d / H broadcast to [B, H, W, C]"""
    B, W, C = d.shape
    dx = _like(d, B, H, W, C)
    check(lib.htrvt_van_hpool_bwd(ptr(d), ptr(dx), B, H, W, C, dt(d.dtype), stream()), "van_hpool_bwd")
    return dx


# ---- Swin fork (csrc/swin.hip): WindowAttention2D, SwinBlock2D, HeightOnlyPatchMerging and Combining of ------------------
# model_sgm_mms_swin/model/HTR_VT.py.  Activations are rows [B*H*W, C] in plain token order (b, h, w), float32 or bfloat16;
# P holds a module's parameters by the fork's names, the Linear / Conv2d weights as [out, in] in the activations' dtype and
# everything else float32 as stored.  Only the attention is a kernel of its own: the rest is layernorm_fwd / _bwd, the
# GEMM with its bias / GELU / residual epilogues, linear_wgrad, the element-wise GELU backward and height_pool_fwd / _bwd.

def win2d_attention_fwd(qkv, table, B, H, W, h, window, shift):
    """attention inside window = (wh, ww) windows of the [H, W] token map rolled by -shift, with the bias of `table`
    (float32 [(2wh-1)(2ww-1), h]) and the fork's additive -100 mask between the wrapped regions -> out [B*H*W, D]"""
    D, hd = _heads(qkv, h)
    out = _like(qkv, B * H * W, D)
    check(lib.htrvt_attn_win2d_fwd(ptr(qkv), ptr(table), ptr(out), B, H, W, h, hd, window[0], window[1], shift[0], shift[1],
                                   hd ** -0.5, dt(qkv.dtype), stream()), "attn_win2d_fwd")
    return out


def win2d_attention_bwd(qkv, table, dout, B, H, W, h, window, shift, dtable=None):
    """dqkv by the recomputing backward; dtable (float32, the table's shape) += the kernel's partial rows, added in row
    order, None: the table gradient is dropped.  The rows are at most 256 and a table has any number of entries (630 in
    the fork; htrvt_colsum takes columns in fours), so they go through htrvt_rowsum_f32, the ordered row sum that is
    htrvt_colsum's own second stage"""
    hd = _heads(qkv, h)[1]
    rows = lib.htrvt_attn_win2d_rows(B, H, W, h, window[0], window[1])
    if rows < 0:
        check(-1, "attn_win2d_rows")
    dqkv = torch.empty_like(qkv)
    partial = _f32(qkv, rows, table.numel())
    check(lib.htrvt_attn_win2d_bwd(ptr(qkv), ptr(table), ptr(dout), ptr(dqkv), ptr(partial), B, H, W, h, hd, window[0],
                                   window[1], shift[0], shift[1], hd ** -0.5, dt(qkv.dtype), stream()), "attn_win2d_bwd")
    if dtable is not None:
        check(lib.htrvt_rowsum_f32(ptr(partial), rows, table.numel(), ptr(dtable), stream()), "rowsum_f32")
    return dqkv


def _gelu_bwd(dy, pre):
    """dy * gelu'(pre), exact (erf) GELU"""
    dpre = torch.empty_like(pre)
    check(lib.htrvt_van_bn_res_gelu_bwd(ptr(dy), ptr(pre), None, None, None, ptr(dpre), pre.shape[0], pre.shape[1], dt(pre.dtype),
                                        stream()), "van_bn_res_gelu_bwd")
    return dpre


def _ln_bwd(dy, x, mean, rstd, gamma, dres=None):
    """(dx (+ dres), dgamma, dbeta)"""
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
    return layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dres=dres), dgamma, dbeta


def swin_block_fwd(x, P, B, H, W, h, window, shift, eps=1e-5, save=True):
    """SwinBlock2D on x [B*H*W, C]: x1 = x + proj(attention(qkv(norm1(x)))), y = x1 + mlp.3(gelu(mlp.0(norm2(x1)))) ->
    (y, saved)"""
    n1, mean1, rstd1 = layernorm_fwd(x, P["norm1.weight"], P["norm1.bias"], eps, save)
    qkv = _pw(n1, P["attn.qkv.weight"], bias=P["attn.qkv.bias"])
    a = win2d_attention_fwd(qkv, P["attn.relative_position_bias_table"], B, H, W, h, window, shift)
    x1 = _pw(a, P["attn.proj.weight"], bias=P["attn.proj.bias"], residual=x)
    n2, mean2, rstd2 = layernorm_fwd(x1, P["norm2.weight"], P["norm2.bias"], eps, save)
    pre = _like(x, x.shape[0], P["mlp.0.weight"].shape[0])
    hid = _pw(n2, P["mlp.0.weight"], bias=P["mlp.0.bias"], act=1, preact=pre)
    y = _pw(hid, P["mlp.3.weight"], bias=P["mlp.3.bias"], residual=x1)
    return y, (n1, mean1, rstd1, qkv, a, x1, n2, mean2, rstd2, pre, hid)


def swin_block_bwd(dy, x, P, saved, B, H, W, h, window, shift):
    """dy [B*H*W, C] -> (dx, {parameter gradients by the fork's names, float32})"""
    n1, mean1, rstd1, qkv, a, x1, n2, mean2, rstd2, pre, hid = saved
    G = {}
    G["mlp.3.weight"], G["mlp.3.bias"] = _pw_wgrad(dy, hid)
    dpre = _gelu_bwd(_pw_dgrad(dy, P["mlp.3.weight"]), pre)
    G["mlp.0.weight"], G["mlp.0.bias"] = _pw_wgrad(dpre, n2)
    dx1, G["norm2.weight"], G["norm2.bias"] = _ln_bwd(_pw_dgrad(dpre, P["mlp.0.weight"]), x1, mean2, rstd2, P["norm2.weight"],
                                                      dres=dy)
    G["attn.proj.weight"], G["attn.proj.bias"] = _pw_wgrad(dx1, a)
    table = P["attn.relative_position_bias_table"]
    G["attn.relative_position_bias_table"] = torch.zeros_like(table)
    dqkv = win2d_attention_bwd(qkv, table, _pw_dgrad(dx1, P["attn.proj.weight"]), B, H, W, h, window, shift,
                               dtable=G["attn.relative_position_bias_table"])
    G["attn.qkv.weight"], G["attn.qkv.bias"] = _pw_wgrad(dqkv, n1)
    dx, G["norm1.weight"], G["norm1.bias"] = _ln_bwd(_pw_dgrad(dqkv, P["attn.qkv.weight"]), x, mean1, rstd1, P["norm1.weight"],
                                                     dres=dx1)
    return dx, G


def _row_planes(x, B, H, W):
    """x [B*H*W, C], H even -> the rows of the even and of the odd map rows, each [B*(H/2)*W, C] (strided copies)"""
    C = x.shape[1]
    x5 = x.view(B, H // 2, 2, W, C)
    return x5[:, :, 0].contiguous().view(-1, C), x5[:, :, 1].contiguous().view(-1, C)


def patch_merge_fwd(x, P, B, H, W, eps=1e-5, save=True):
    """HeightOnlyPatchMerging on x [B*H*W, C]: norm(W0 x[b, 2h', w] + W1 x[b, 2h' + 1, w]), the Conv2d(C, Cout, (2, 1),
    stride (2, 1), bias=False) as two products over the gathered even / odd map rows, the second taking the first as its
    residual.  P["reduce.weight"]: (W0, W1), each [Cout, C] -> (y [B*(H/2)*W, Cout], saved)"""
    xe, xo = _row_planes(x, B, H, W)
    w0, w1 = P["reduce.weight"]
    z = _pw(xo, w1, residual=_pw(xe, w0))
    y, mean, rstd = layernorm_fwd(z, P["norm.weight"], P["norm.bias"], eps, save)
    return y, (xe, xo, z, mean, rstd)


def patch_merge_bwd(dy, P, saved, B, H, W):
    """dy [B*(H/2)*W, Cout] -> (dx [B*H*W, C], {"reduce.weight": float32 [Cout, C, 2, 1], "norm.weight", "norm.bias"})"""
    xe, xo, z, mean, rstd = saved
    w0, w1 = P["reduce.weight"]
    dz, dgamma, dbeta = _ln_bwd(dy, z, mean, rstd, P["norm.weight"])
    dw = torch.stack((_pw_wgrad(dz, xe, bias=False)[0], _pw_wgrad(dz, xo, bias=False)[0]), dim=2).unsqueeze(3)
    C = xe.shape[1]
    dx = torch.stack((_pw_dgrad(dz, w0).view(B, H // 2, W, C), _pw_dgrad(dz, w1).view(B, H // 2, W, C)), dim=2)
    return dx.view(B * H * W, C), {"reduce.weight": dw, "norm.weight": dgamma, "norm.bias": dbeta}


def combining_fwd(x, P, B, H, W):
    """Combining on x [B*H*W, C]: gelu(fc(mean over H)) -> (y [B*W, Cout], saved)"""
    pooled = height_pool_fwd(x.view(B, H, W, x.shape[1])).view(B * W, x.shape[1])
    pre = _like(x, B * W, P["fc.weight"].shape[0])
    y = _pw(pooled, P["fc.weight"], bias=P["fc.bias"], act=1, preact=pre)
    return y, (pooled, pre)


def combining_bwd(dy, P, saved, B, H, W):
    """dy [B*W, Cout] -> (dx [B*H*W, C], {"fc.weight", "fc.bias"})"""
    pooled, pre = saved
    dpre = _gelu_bwd(dy, pre)
    dw, db = _pw_wgrad(dpre, pooled)
    dx = height_pool_bwd(_pw_dgrad(dpre, P["fc.weight"]).view(B, W, pooled.shape[1]), H)
    return dx.view(B * H * W, pooled.shape[1]), {"fc.weight": dw, "fc.bias": db}


def window_attention_fwd(x, P, Bn, h, window):
    """WindowAttention2D on partitioned windows x [Bn*wh*ww, C] without a mask: proj(attention(qkv(x))), every window a map
    of its own -> (y, saved)"""
    qkv = _pw(x, P["qkv.weight"], bias=P["qkv.bias"])
    a = win2d_attention_fwd(qkv, P["relative_position_bias_table"], Bn, window[0], window[1], h, window, (0, 0))
    return _pw(a, P["proj.weight"], bias=P["proj.bias"]), (qkv, a)


def window_attention_bwd(dy, x, P, saved, Bn, h, window):
    qkv, a = saved
    G = {}
    G["proj.weight"], G["proj.bias"] = _pw_wgrad(dy, a)
    table = P["relative_position_bias_table"]
    G["relative_position_bias_table"] = torch.zeros_like(table)
    dqkv = win2d_attention_bwd(qkv, table, _pw_dgrad(dy, P["proj.weight"]), Bn, window[0], window[1], h, window, (0, 0),
                               dtable=G["relative_position_bias_table"])
    G["qkv.weight"], G["qkv.bias"] = _pw_wgrad(dqkv, x)
    return _pw_dgrad(dqkv, P["qkv.weight"]), G


# ---- SVTR fork (csrc/svtr.hip): MultiHeadSelfAttention, MixingBlock and Merging of model_sgm_mms_svtr/model/svtr.py (its -----
# Combining is the Swin fork's: combining_fwd / _bwd above).  Rows and P as in the Swin section; the fork's qkv Linear has no
# bias.  A local block's attention is the neighbourhood kernel; a global block's is the fused kernel of csrc/attention.hip in
# bfloat16 and the unfused GEMM route otherwise.

def nbr2d_attention_fwd(qkv, B, H, W, h, kernel, save=True):
    """every query (y, x) of the [H, W] token map over the keys of its centred kernel = (kh, kw) box, clipped to the map ->
    (out [B*H*W, D], lse float32 [B*h, H*W] or None)"""
    D, hd = _heads(qkv, h)
    out = _like(qkv, B * H * W, D)
    lse = _f32(qkv, B * h, H * W) if save else None
    check(lib.htrvt_attn_nbr2d_fwd(ptr(qkv), ptr(out), ptr(lse), B, H, W, h, hd, kernel[0], kernel[1], hd ** -0.5,
                                   dt(qkv.dtype), stream()), "attn_nbr2d_fwd")
    return out, lse


def nbr2d_attention_bwd(qkv, out, dout, lse, B, H, W, h, kernel):
    """dqkv by the recomputing backward (two launches: dq, then dk / dv); no workspace"""
    hd = _heads(qkv, h)[1]
    dqkv = torch.empty_like(qkv)
    check(lib.htrvt_attn_nbr2d_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), B, H, W, h, hd, kernel[0], kernel[1],
                                   hd ** -0.5, dt(qkv.dtype), stream()), "attn_nbr2d_bwd")
    return dqkv


def _global_fused(qkv, N):
    """a global block's route: the fused kernel serves bfloat16 and N >= 32"""
    return qkv.dtype == torch.bfloat16 and N >= 32


def _mixing_attention_fwd(qkv, B, H, W, h, kernel, save):
    """-> (a, what the backward takes: lse, or the unfused route's P)"""
    if kernel is not None:
        return nbr2d_attention_fwd(qkv, B, H, W, h, kernel, save)
    if _global_fused(qkv, H * W):
        return attention_fwd(qkv, B, H * W, h, save=save)
    return attention_unfused_fwd(qkv, B, H * W, h)


def _mixing_attention_bwd(qkv, a, da, aux, B, H, W, h, kernel):
    if kernel is not None:
        return nbr2d_attention_bwd(qkv, a, da, aux, B, H, W, h, kernel)
    if _global_fused(qkv, H * W):
        return attention_bwd(qkv, a, da, aux, B, H * W, h)
    return attention_unfused_bwd(qkv, aux, da, B, H * W, h)


def mha_fwd(x, P, B, H, W, h, kernel, save=True):
    """MultiHeadSelfAttention on x [B*H*W, C]: proj(attention(qkv(x))), kernel = (kh, kw) for a local module, None for a
    global one -> (y, saved)"""
    qkv = _pw(x, P["qkv.weight"])
    a, aux = _mixing_attention_fwd(qkv, B, H, W, h, kernel, save)
    return _pw(a, P["proj.weight"], bias=P["proj.bias"]), (qkv, a, aux)


def mha_bwd(dy, x, P, saved, B, H, W, h, kernel):
    qkv, a, aux = saved
    G = {}
    G["proj.weight"], G["proj.bias"] = _pw_wgrad(dy, a)
    dqkv = _mixing_attention_bwd(qkv, a, _pw_dgrad(dy, P["proj.weight"]), aux, B, H, W, h, kernel)
    G["qkv.weight"] = _pw_wgrad(dqkv, x, bias=False)[0]
    return _pw_dgrad(dqkv, P["qkv.weight"]), G


def mixing_block_fwd(x, P, B, H, W, h, kernel, eps=1e-5, save=True):
    """MixingBlock on x [B*H*W, C]: x1 = x + proj(attention(qkv(norm1(x)))), y = x1 + mlp.2(gelu(mlp.0(norm2(x1)))) ->
    (y, saved).  kernel = (kh, kw): a local block, the neighbourhood kernel.  kernel = None: a global block -- bfloat16 with
    H*W >= 32 through the fused attention kernel, float32 (and bfloat16 with fewer than 32 tokens) through the unfused
    route, which keeps a [B*h, N, N] P for the backward and is the parity route only"""
    n1, mean1, rstd1 = layernorm_fwd(x, P["norm1.weight"], P["norm1.bias"], eps, save)
    qkv = _pw(n1, P["attn.qkv.weight"])
    a, aux = _mixing_attention_fwd(qkv, B, H, W, h, kernel, save)
    x1 = _pw(a, P["attn.proj.weight"], bias=P["attn.proj.bias"], residual=x)
    n2, mean2, rstd2 = layernorm_fwd(x1, P["norm2.weight"], P["norm2.bias"], eps, save)
    pre = _like(x, x.shape[0], P["mlp.0.weight"].shape[0])
    hid = _pw(n2, P["mlp.0.weight"], bias=P["mlp.0.bias"], act=1, preact=pre)
    y = _pw(hid, P["mlp.2.weight"], bias=P["mlp.2.bias"], residual=x1)
    return y, (n1, mean1, rstd1, qkv, a, aux, x1, n2, mean2, rstd2, pre, hid)


def mixing_block_bwd(dy, x, P, saved, B, H, W, h, kernel):
    """dy [B*H*W, C] -> (dx, {parameter gradients by the fork's names, float32})"""
    n1, mean1, rstd1, qkv, a, aux, x1, n2, mean2, rstd2, pre, hid = saved
    G = {}
    G["mlp.2.weight"], G["mlp.2.bias"] = _pw_wgrad(dy, hid)
    dpre = _gelu_bwd(_pw_dgrad(dy, P["mlp.2.weight"]), pre)
    G["mlp.0.weight"], G["mlp.0.bias"] = _pw_wgrad(dpre, n2)
    dx1, G["norm2.weight"], G["norm2.bias"] = _ln_bwd(_pw_dgrad(dpre, P["mlp.0.weight"]), x1, mean2, rstd2, P["norm2.weight"],
                                                      dres=dy)
    G["attn.proj.weight"], G["attn.proj.bias"] = _pw_wgrad(dx1, a)
    dqkv = _mixing_attention_bwd(qkv, a, _pw_dgrad(dx1, P["attn.proj.weight"]), aux, B, H, W, h, kernel)
    G["attn.qkv.weight"] = _pw_wgrad(dqkv, n1, bias=False)[0]
    dx, G["norm1.weight"], G["norm1.bias"] = _ln_bwd(_pw_dgrad(dqkv, P["attn.qkv.weight"]), x, mean1, rstd1, P["norm1.weight"],
                                                     dres=dx1)
    return dx, G


def svtr_merge_geom(B, H, W, Ci, Co):
    """the Merging convolution: 3x3, stride (2, 1), padding 1 on the NHWC map; Ho = (H - 1) // 2 + 1"""
    return ConvGeom(B, H, W, Ci, Co, 3, (2, 1), 1)


def svtr_merge_packs(w, dtype):
    """Conv2d weight [Co, Ci, 3, 3] -> the conv gather descriptors' operands (torch copies): the forward pack
    [Co][9][cpad(Ci)] and the dgrad pack [Ci][9][cpad(Co)], tap = 3 ky + kx, the padding channels zero"""
    Co, Ci = w.shape[:2]
    taps = w.reshape(Co, Ci, 9)
    fwd = torch.zeros(Co, 9, cpad(Ci, dtype), dtype=dtype, device=w.device)
    dgr = torch.zeros(Ci, 9, cpad(Co, dtype), dtype=dtype, device=w.device)
    fwd[:, :, :Ci] = taps.permute(0, 2, 1)
    dgr[:, :, :Co] = taps.permute(1, 2, 0)
    return fwd, dgr


def _dgrad_by_class(g, dtype):
    """one launch per input-row parity class, each over the taps that reach it: the form the bfloat16 LDS-DMA kernels
    serve, for classes of more than 128 pixels; otherwise one launch over every pixel and tap"""
    return dtype == torch.bfloat16 and all(g.B * Hq * Wq > 128 for _a, _b, _nt, Hq, Wq in g.parity_classes())


def svtr_merge_fwd(x, P, B, H, W, eps=1e-5, save=True):
    """Merging on x [B*H*W, C], which is the NHWC map: norm(conv(x) + bias) with the convolution gathered by htrvt_gemm
    (GATHER_CONV_FWD), the bias in its epilogue.  P["conv.weight"]: (forward pack, dgrad pack) of svtr_merge_packs ->
    (y [B*Ho*W, Cout], saved)"""
    wf = P["conv.weight"][0]
    g = svtr_merge_geom(B, H, W, x.shape[1], wf.shape[0])
    cpi = cpad(g.Ci, x.dtype)
    z = _like(x, B * g.Ho * g.Wo, g.Co)
    gemm(x, wf, z, dtype=x.dtype, M=B * g.Ho * g.Wo, N=g.Co, K=g.taps * cpi, lda=g.Ci, ldb=g.taps * cpi, ldc=g.Co,
         gather=GATHER_CONV_FWD, geom=g, Cpad=cpi, bias=P["conv.bias"])
    y, mean, rstd = layernorm_fwd(z, P["norm.weight"], P["norm.bias"], eps, save)
    return y, (z, mean, rstd)


def svtr_merge_bwd(dy, x, P, saved, B, H, W):
    """dy [B*Ho*W, Cout] -> (dx [B*H*W, C], {"conv.weight": float32 [Cout, C, 3, 3], "conv.bias", "norm.weight",
    "norm.bias"}): the weight gradient by GATHER_CONV_WGRAD in the descriptor's [9][cpad(C)][Cout] form and copied back, the
    bias gradient the column sums of dz, dx by GATHER_CONV_DGRAD"""
    z, mean, rstd = saved
    wd = P["conv.weight"][1]
    g = svtr_merge_geom(B, H, W, x.shape[1], z.shape[1])
    M = B * g.Ho * g.Wo
    cpi, cpo = cpad(g.Ci, x.dtype), cpad(g.Co, x.dtype)
    dz, dgamma, dbeta = _ln_bwd(dy, z, mean, rstd, P["norm.weight"])
    db = torch.zeros(g.Co, dtype=torch.float32, device=x.device)
    colsum(dz, M, g.Co, g.Co, db, dti=dt(dz.dtype))
    packed = torch.zeros(g.taps, cpi, g.Co, dtype=torch.float32, device=x.device)
    gemm(x, dz, packed, dtype=x.dtype, M=g.taps * cpi, N=g.Co, K=M, lda=g.Ci, ldb=g.Co, ldc=g.Co, a_layout=MNMAJOR,
         b_layout=MNMAJOR, gather=GATHER_CONV_WGRAD, geom=g, Cpad=cpi, accumulate=True, c_f32=True)
    dw = packed[:, :g.Ci].permute(2, 1, 0).reshape(g.Co, g.Ci, 3, 3).contiguous()
    dx = _like(x, B * H * W, g.Ci)
    kw = dict(dtype=x.dtype, N=g.Ci, lda=g.Co, ldb=g.taps * cpo, ldc=g.Ci, gather=GATHER_CONV_DGRAD, geom=g, Cpad=cpo)
    if _dgrad_by_class(g, x.dtype):
        for a, b, nt, Hq, Wq in g.parity_classes():
            gemm(dz, wd, dx, M=B * Hq * Wq, K=nt * cpo, cls=(a, b), **kw)
    else:
        gemm(dz, wd, dx, M=B * H * W, K=g.taps * cpo, **kw)
    return dx, {"conv.weight": dw, "conv.bias": db, "norm.weight": dgamma, "norm.bias": dbeta}


# ---- convolutional forks (csrc/gnmixer.hip): ConvModule, FeedForward, SqueezeExcite1D, Downsample1D, Upsample1D and the
# blocks of model_sgm_mms_conv/model/HTR_VT.py and model_sgm_mms_conv_squeeze/model/HTR_VT.py on rows [B*N, D].  P maps the
# fork's parameter names to tensors: Linear and 1x1 Conv1d weights as [out, in] in the activations' dtype, everything else
# (biases, norms, the depthwise weight [C, 1, k], the excite MLP) float32 as stored.

def gn_mixer_fwd(u, weight, bias, gamma, beta, B, N, eps=1e-5):
    """u [B*N, 2*C] (pointwise_conv1's output), weight float32 [C, 1, k] -> (s [B*N, C], (c, mean, rstd)):
    s = silu(GroupNorm(1, C)(dwconv(glu(u)) + bias)), the statistics float32 [B] over the C * N values of each image"""
    C, k, dti, st = u.shape[1] // 2, weight.shape[-1], dt(u.dtype), stream()
    parts = lib.htrvt_gnmixer_parts(B, N, C, dti)
    if parts < 0:
        check(-1, "gnmixer_fwd")
    c, pairs, mean, rstd = _like(u, B * N, C), _f32(u, B, parts, 2), _f32(u, B), _f32(u, B)
    check(lib.htrvt_gnmixer_fwd(ptr(u), ptr(weight), ptr(bias), ptr(c), ptr(pairs), B, N, C, k, dti, st), "gnmixer_fwd")
    check(lib.htrvt_gn_finalize(ptr(pairs), B, parts, float(C * N), eps, ptr(mean), ptr(rstd), st), "gn_finalize")
    return gn_mixer_act(c, mean, rstd, gamma, beta, B, N), (c, mean, rstd)


def gn_mixer_act(c, mean, rstd, gamma, beta, B, N, s=None):
    """s = silu((c - mean_b) * rstd_b * gamma + beta): the forward's last pass, and the backward's way to s without keeping it"""
    s = torch.empty_like(c) if s is None else s
    check(lib.htrvt_gnmixer_act(ptr(c), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(s), B, N, c.shape[1], dt(c.dtype),
                                stream()), "gnmixer_act")
    return s


def gn_mixer_bwd(ds, u, weight, gamma, beta, B, N, saved):
    """ds [B*N, C] -> (du [B*N, 2*C], dweight [C, 1, k], dbias, dgamma, dbeta), float32 parameter gradients"""
    c, mean, rstd = saved
    C, k, dti, st = u.shape[1] // 2, weight.shape[-1], dt(u.dtype), stream()
    rows, parts = lib.htrvt_gnmixer_rows(B, N, C, dti), lib.htrvt_gnmixer_parts(B, N, C, dti)
    if rows < 0 or parts < 0:
        check(-1, "gnmixer_bwd")
    pc, pairs, m1, m2 = _f32(u, rows, 2 * C), _f32(u, B, parts, 2), _f32(u, B), _f32(u, B)
    check(lib.htrvt_gnmixer_bwd_reduce(ptr(ds), ptr(c), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(pc), ptr(pairs), B, N, C,
                                       dti, st), "gnmixer_bwd_reduce")
    check(lib.htrvt_gn_bwd_finalize(ptr(pairs), B, parts, float(C * N), ptr(m1), ptr(m2), st), "gn_bwd_finalize")
    dnorm = torch.zeros(2 * C, dtype=torch.float32, device=u.device)       # (d beta | d gamma): one column-sum launch
    colsum(pc, rows, 2 * C, 2 * C, dnorm, dti=0)
    pw, pb, du = _f32(u, rows, C * k), _f32(u, rows, C), torch.empty_like(u)
    check(lib.htrvt_gnmixer_bwd(ptr(u), ptr(c), ptr(ds), ptr(weight), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(m1),
                                ptr(m2), ptr(du), ptr(pw), ptr(pb), B, N, C, k, dti, st), "gnmixer_bwd")
    dweight = torch.zeros_like(weight)
    colsum(pw, rows, C * k, C * k, dweight, dti=0)
    dbias = torch.zeros(C, dtype=torch.float32, device=u.device)
    colsum(pb, rows, C, C, dbias, dti=0)
    return du, dweight, dbias, dnorm[C:], dnorm[:C]


def se_fwd(x, w1, b1, w2, b2, B, N):
    """SqueezeExcite1D on x [B*N, D]: y = x * g[b], g = sigmoid(fc2(silu(fc1(mean over the tokens)))); the MLP (w1 [H, D],
    w2 [D, H], float32) runs in float32 -> (y, (mean [B, D], pre [B, H], act [B, H], g [B, D]))"""
    D, H, dti, st = x.shape[1], w1.shape[0], dt(x.dtype), stream()
    mean, pre, act, g, y = _f32(x, B, D), _f32(x, B, H), _f32(x, B, H), _f32(x, B, D), torch.empty_like(x)
    check(lib.htrvt_se_mean(ptr(x), ptr(mean), B, N, D, dti, st), "se_mean")
    check(lib.htrvt_se_mlp_fwd(ptr(mean), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(pre), ptr(act), ptr(g), B, D, H, st), "se_mlp_fwd")
    check(lib.htrvt_se_scale_fwd(ptr(x), ptr(g), ptr(y), B, N, D, dti, st), "se_scale_fwd")
    return y, (mean, pre, act, g)


def se_bwd(dy, x, w1, w2, B, N, saved):
    """dy [B*N, D] -> (dx, (dw1, db1, dw2, db2)), the weight gradients summed over the images in order"""
    mean, pre, act, g = saved
    D, H, dti, st = x.shape[1], w1.shape[0], dt(x.dtype), stream()
    dg, dh2, dh1, dmean = _f32(x, B, D), _f32(x, B, D), _f32(x, B, H), _f32(x, B, D)
    check(lib.htrvt_se_scale_bwd_reduce(ptr(dy), ptr(x), ptr(dg), B, N, D, dti, st), "se_scale_bwd_reduce")
    check(lib.htrvt_se_mlp_bwd(ptr(dg), ptr(g), ptr(pre), ptr(w1), ptr(w2), ptr(dh2), ptr(dh1), ptr(dmean), B, D, H, st), "se_mlp_bwd")
    dw2, db2, dw1, db1 = _f32(x, D, H), _f32(x, D), _f32(x, H, D), _f32(x, H)
    check(lib.htrvt_se_wgrad(ptr(dh2), ptr(act), ptr(dw2), ptr(db2), B, D, H, st), "se_wgrad")
    check(lib.htrvt_se_wgrad(ptr(dh1), ptr(mean), ptr(dw1), ptr(db1), B, H, D, st), "se_wgrad")
    dx = torch.empty_like(x)
    check(lib.htrvt_se_scale_bwd(ptr(dy), ptr(g), ptr(dmean), ptr(dx), B, N, D, dti, st), "se_scale_bwd")
    return dx, (dw1, db1, dw2, db2)


def seq_down2_fwd(x, B, N):
    """Downsample1D on x [B*N, D]: the mean of tokens 2j and 2j + 1 -> [B*(N // 2), D]; N <= 1 is the identity"""
    if N <= 1:
        return x
    y = _like(x, B * (N // 2), x.shape[1])
    check(lib.htrvt_seq_down2_fwd(ptr(x), ptr(y), B, N, x.shape[1], dt(x.dtype), stream()), "seq_down2_fwd")
    return y


def seq_down2_bwd(dy, B, N):
    """dy [B*(N // 2), D] -> dx [B*N, D]; an odd last token gets zero"""
    if N <= 1:
        return dy
    dx = _like(dy, B * N, dy.shape[1])
    check(lib.htrvt_seq_down2_bwd(ptr(dy), ptr(dx), B, N, dy.shape[1], dt(dy.dtype), stream()), "seq_down2_bwd")
    return dx


def seq_up_add_fwd(y, skip, B, n, N0):
    """Upsample1D fused with the encoder's skip add: out[b, i] = y[b, (i * n) // N0] + skip[b, i] -> [B*N0, D]"""
    out = torch.empty_like(skip)
    check(lib.htrvt_seq_up_add_fwd(ptr(y), ptr(skip), ptr(out), B, n, N0, y.shape[1], dt(y.dtype), stream()), "seq_up_add_fwd")
    return out


def seq_up_add_bwd(dout, B, n, N0):
    """dout [B*N0, D] -> dy [B*n, D], each source token's targets summed in order (the skip's gradient is dout itself)"""
    dy = _like(dout, B * n, dout.shape[1])
    check(lib.htrvt_seq_up_add_bwd(ptr(dout), ptr(dy), B, n, N0, dout.shape[1], dt(dout.dtype), stream()), "seq_up_add_bwd")
    return dy


def silu(pre):
    a = torch.empty_like(pre)
    check(lib.htrvt_silu_fwd(ptr(pre), ptr(a), pre.numel(), dt(pre.dtype), stream()), "silu_fwd")
    return a


def silu_bwd(da, pre):
    dpre = torch.empty_like(pre)
    check(lib.htrvt_silu_bwd(ptr(da), ptr(pre), ptr(dpre), pre.numel(), dt(pre.dtype), stream()), "silu_bwd")
    return dpre


def silu_ffn_fwd(x, w1, b1, w2, b2, alpha=1.0, residual=None):
    """FeedForward on x [rows, D]: alpha * lin2(silu(lin1(x))) (+ residual) -> (y, (pre,)); alpha rides in the second GEMM's
    descriptor (the bias scaled to match), the activation is kept as lin1's output only"""
    pre = _pw(x, w1, bias=b1)
    y = _pw(silu(pre), w2, bias=b2 if alpha == 1.0 else b2 * alpha, alpha=alpha, residual=residual)
    return y, (pre,)


def silu_ffn_bwd(dy, x, w1, w2, saved, alpha=1.0):
    """dy [rows, D] (the gradient at y) -> (dx, (dw1, db1, dw2, db2))"""
    (pre,) = saved
    dw2, db2 = _pw_wgrad(dy, silu(pre))
    if alpha != 1.0:
        dw2, db2 = dw2.mul_(alpha), db2.mul_(alpha)
    dpre = silu_bwd(_pw_dgrad(dy, w2, alpha=alpha), pre)
    dw1, db1 = _pw_wgrad(dpre, x)
    return _pw_dgrad(dpre, w1), (dw1, db1, dw2, db2)


def _sub(P, prefix):
    return {n[len(prefix):]: t for n, t in P.items() if n.startswith(prefix)}


def _put(G, prefix, names, grads):
    for n, g in zip(names, grads):
        G[prefix + n] = g


FFN_NAMES = ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias")


# The regularisers of a residual site are `(p, p_path, seeds)`: element-wise dropout p on the branch, drop-path p_path on
# whole samples, seeds an int64 device tensor of two elements (residual_dropout's keys), None when both rates are 0.  A
# backward takes the forward's.  None stands for a site, or a whole block, without regularisers: the launches without them.

def _site_on(site):
    return site is not None and (site[0] > 0 or site[1] > 0)


def _conv_branch_fwd(t, P, B, N, gn_eps, residual=None):
    """pointwise_conv2(silu(GroupNorm(dwconv(glu(pointwise_conv1(t)))))) (+ residual, in the last GEMM's epilogue) on the
    normed rows t -> (o, (u, c, gn_mean, gn_rstd))"""
    u = _pw(t, P["pointwise_conv1.weight"], bias=P["pointwise_conv1.bias"])
    s, gn = gn_mixer_fwd(u, P["depthwise_conv.weight"], P["depthwise_conv.bias"], P["norm.weight"], P["norm.bias"], B, N, gn_eps)
    return _pw(s, P["pointwise_conv2.weight"], bias=P["pointwise_conv2.bias"], residual=residual), (u,) + gn


def _conv_branch_bwd(do, t, P, saved, B, N):
    """do [B*N, D], the gradient at the branch's output -> (dt, {the branch's parameter gradients})"""
    u, c, gmean, grstd = saved
    G = {}
    s = gn_mixer_act(c, gmean, grstd, P["norm.weight"], P["norm.bias"], B, N)
    G["pointwise_conv2.weight"], G["pointwise_conv2.bias"] = _pw_wgrad(do, s)
    du, G["depthwise_conv.weight"], G["depthwise_conv.bias"], G["norm.weight"], G["norm.bias"] = gn_mixer_bwd(
        _pw_dgrad(do, P["pointwise_conv2.weight"]), u, P["depthwise_conv.weight"], P["norm.weight"], P["norm.bias"], B, N,
        (c, gmean, grstd))
    G["pointwise_conv1.weight"], G["pointwise_conv1.bias"] = _pw_wgrad(du, t)
    return _pw_dgrad(du, P["pointwise_conv1.weight"]), G


def conv_module_fwd(x, P, B, N, eps=1e-5, gn_eps=1e-5, drop=None, save=True):
    """ConvModule on x [B*N, D]: x + drop_path(dropout(pointwise_conv2(silu(GroupNorm(dwconv(glu(pointwise_conv1(
    LayerNorm(x))))))))).  drop: None or the site's (p, p_path, seeds) ->
    (y, (t, mean, rstd, u, c, gn_mean, gn_rstd))"""
    t, mean, rstd = layernorm_fwd(x, P["layer_norm.weight"], P["layer_norm.bias"], eps, save)
    if not _site_on(drop):
        y, bs = _conv_branch_fwd(t, P, B, N, gn_eps, residual=x)
    else:
        o, bs = _conv_branch_fwd(t, P, B, N, gn_eps)
        y = residual_dropout(o, x, N, drop[2], drop[0], drop[1])
    return y, (t, mean, rstd) + bs


def conv_module_bwd(dy, x, P, saved, B, N, drop=None):
    """dy [B*N, D] -> (dx, {parameter gradients by the fork's names, float32})"""
    t, mean, rstd = saved[:3]
    do = dy if not _site_on(drop) else residual_dropout(dy, None, N, drop[2], drop[0], drop[1])
    dt_, G = _conv_branch_bwd(do, t, P, saved[3:], B, N)
    dx, G["layer_norm.weight"], G["layer_norm.bias"] = _ln_bwd(dt_, x, mean, rstd, P["layer_norm.weight"], dres=dy)
    return dx, G


def _padded_tokens(qkv, N):
    """the unfused route's row length: N as it is where its GEMMs take it (16-byte rows), else the next such length"""
    a = 8 if qkv.dtype == torch.bfloat16 else 4
    return (N + a - 1) // a * a


def _pad_tokens(x, B, N, Np):
    xp = torch.zeros(B, Np, x.shape[1], dtype=x.dtype, device=x.device)
    xp[:, :N] = x.view(B, N, x.shape[1])
    return xp.view(B * Np, x.shape[1])


def plain_attention_pads(dtype, N):
    """whether the blocks' attention at N tokens takes the unfused route with a padded token count (no dropout there)"""
    a = 8 if dtype == torch.bfloat16 else 4
    return not (dtype == torch.bfloat16 and N >= 32) and N % a != 0


def plain_attention_fwd(qkv, B, N, h, save=True, drop=None):
    """the blocks' attention -> (a [B*N, D], aux): the fused kernel in bfloat16 with N >= 32 (aux = lse), else the unfused
    GEMM route (aux = P), the parity route; there a token count off the 16-byte row is padded with keys masked by a -1e30
    score bias (torch copies in and out).  drop: (seed, p) on the probabilities, the same mask on the fused and the unfused
    route; the padded route has another element order and refuses it"""
    if _global_fused(qkv, N):
        return attention_fwd(qkv, B, N, h, save=save, drop=drop)
    Np = _padded_tokens(qkv, N)
    if Np == N:
        return attention_unfused_fwd(qkv, B, N, h, drop=drop)
    if drop is not None:
        raise NotImplementedError(f"attention dropout p = {drop[1]} at N = {N} tokens: the unfused route pads N to {Np} and does "
                                  "not draw a mask there")
    bias = torch.zeros(h, Np, Np, dtype=torch.float32, device=qkv.device)
    bias[:, :, N:] = -1e30
    out, P = attention_unfused_fwd(_pad_tokens(qkv, B, N, Np), B, Np, h, bias=bias)
    return out.view(B, Np, -1)[:, :N].reshape(B * N, -1), P


def plain_attention_bwd(qkv, a, da, aux, B, N, h, drop=None):
    if _global_fused(qkv, N):
        return attention_bwd(qkv, a, da, aux, B, N, h, drop=drop)
    Np = _padded_tokens(qkv, N)
    if Np == N:
        return attention_unfused_bwd(qkv, aux, da, B, N, h, drop=drop)
    dqkv = attention_unfused_bwd(_pad_tokens(qkv, B, N, Np), aux, _pad_tokens(da, B, N, Np), B, Np, h)
    return dqkv.view(B, Np, -1)[:, :N].reshape(B * N, -1)


BLOCK_SAVED = 31      # entries of a block's `saved`
BlockDrop = collections.namedtuple("BlockDrop", "ffn1 attn conv ffn2 probs")
BlockDrop.__doc__ = """a block's regularisers: the four residual sites' (p, p_path, seeds) in the order of the forward, and
probs = (seed, p) of the dropout on the attention probabilities or None"""


def _block_drops(drops):
    """None when nothing is active, so that the rate-0 launch sequence runs"""
    if drops is None or not (any(_site_on(s) for s in drops[:4]) or drops.probs is not None):
        return None
    return drops


def _add_ln_fwd(branch, res, site, N, gamma, beta, eps, save):
    """a site in the forward: res + drop_path(dropout(branch)) and the next norm, one launch -> (s, y, mean, rstd)"""
    p, p_path, seeds = site if site is not None else (0.0, 0.0, None)
    return drop_add_ln_fwd(branch, res, N, seeds, p, p_path, gamma, beta, eps, save)


def _ln_bwd_drop(dy, s, mean, rstd, gamma, site, N, dres=None):
    """a site in the backward -> (ds, dbranch, dgamma, dbeta)"""
    p, p_path, seeds = site if site is not None else (0.0, 0.0, None)
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
    ds, db = layernorm_bwd_drop(dy, s, mean, rstd, gamma, dgamma, dbeta, N, seeds, p, p_path, dres=dres)
    return ds, db, dgamma, dbeta


def conformer_block_fwd(x, P, B, N, h, eps=1e-5, conv_eps=1e-5, gn_eps=1e-5, squeeze=False, drops=None, save=True):
    """ConformerBlock (squeeze=False) / SqueezeConformerBlock (squeeze=True) on x [B*N, D]:
    x + 1/2 ffn1 -> + attention -> + the ConvModule's branch -> (SE gate) -> + 1/2 ffn2 -> final_norm -> (y, saved).
    drops: None or a BlockDrop.  Without an active regulariser every add rides in the epilogue of the GEMM that ends its
    branch.  With one, that GEMM writes the branch alone (the feed-forwards' 1/2 stays in its alpha: it commutes with the
    masks) and drop_add_ln_fwd forms the new residual stream and the next norm's output in one launch; behind the SE gate of
    the squeeze block the conv site is residual_dropout and the plain norm."""
    drops = _block_drops(drops)
    if drops is not None:
        return _conformer_block_fwd_drop(x, P, B, N, h, eps, conv_eps, gn_eps, squeeze, drops, save)
    n1, m1, r1 = layernorm_fwd(x, P["ffn1_norm.weight"], P["ffn1_norm.bias"], eps, save)
    x1, (pre1,) = silu_ffn_fwd(n1, *[P["ffn1." + n] for n in FFN_NAMES], alpha=0.5, residual=x)
    n2, m2, r2 = layernorm_fwd(x1, P["attn_norm.weight"], P["attn_norm.bias"], eps, save)
    qkv = _pw(n2, P["attn.qkv.weight"], bias=P["attn.qkv.bias"])
    a, aux = plain_attention_fwd(qkv, B, N, h, save)
    x2 = _pw(a, P["attn.proj.weight"], bias=P["attn.proj.bias"], residual=x1)
    x3, cs = conv_module_fwd(x2, _sub(P, "conv_module."), B, N, conv_eps, gn_eps, None, save)
    x4, ss = x3, (None,) * 4
    if squeeze:
        x4, ss = se_fwd(x3, P["se.fc1.weight"], P["se.fc1.bias"], P["se.fc2.weight"], P["se.fc2.bias"], B, N)
    n5, m5, r5 = layernorm_fwd(x4, P["ffn2_norm.weight"], P["ffn2_norm.bias"], eps, save)
    x5, (pre2,) = silu_ffn_fwd(n5, *[P["ffn2." + n] for n in FFN_NAMES], alpha=0.5, residual=x4)
    y, m6, r6 = layernorm_fwd(x5, P["final_norm.weight"], P["final_norm.bias"], eps, save)
    saved = (n1, m1, r1, pre1, x1, n2, m2, r2, qkv, a, aux, x2) + cs + (x3,) + ss + (n5, m5, r5, pre2, x5, m6, r6)
    return y, saved


def _conformer_block_fwd_drop(x, P, B, N, h, eps, conv_eps, gn_eps, squeeze, drops, save):
    """the forward with regularisers; `saved` has the layout of the forward without"""
    Pc = _sub(P, "conv_module.")
    n1, m1, r1 = layernorm_fwd(x, P["ffn1_norm.weight"], P["ffn1_norm.bias"], eps, save)
    b1, (pre1,) = silu_ffn_fwd(n1, *[P["ffn1." + n] for n in FFN_NAMES], alpha=0.5)
    x1, n2, m2, r2 = _add_ln_fwd(b1, x, drops.ffn1, N, P["attn_norm.weight"], P["attn_norm.bias"], eps, save)
    qkv = _pw(n2, P["attn.qkv.weight"], bias=P["attn.qkv.bias"])
    a, aux = plain_attention_fwd(qkv, B, N, h, save, drop=drops.probs)
    b2 = _pw(a, P["attn.proj.weight"], bias=P["attn.proj.bias"])
    x2, t, mc, rc = _add_ln_fwd(b2, x1, drops.attn, N, Pc["layer_norm.weight"], Pc["layer_norm.bias"], conv_eps, save)
    b3, bs = _conv_branch_fwd(t, Pc, B, N, gn_eps)
    if squeeze:
        p, p_path, seeds = drops.conv if drops.conv is not None else (0.0, 0.0, None)
        x3 = residual_dropout(b3, x2, N, seeds, p, p_path)
        x4, ss = se_fwd(x3, P["se.fc1.weight"], P["se.fc1.bias"], P["se.fc2.weight"], P["se.fc2.bias"], B, N)
        n5, m5, r5 = layernorm_fwd(x4, P["ffn2_norm.weight"], P["ffn2_norm.bias"], eps, save)
    else:
        x3, n5, m5, r5 = _add_ln_fwd(b3, x2, drops.conv, N, P["ffn2_norm.weight"], P["ffn2_norm.bias"], eps, save)
        x4, ss = x3, (None,) * 4
    b5, (pre2,) = silu_ffn_fwd(n5, *[P["ffn2." + n] for n in FFN_NAMES], alpha=0.5)
    x5, y, m6, r6 = _add_ln_fwd(b5, x4, drops.ffn2, N, P["final_norm.weight"], P["final_norm.bias"], eps, save)
    saved = (n1, m1, r1, pre1, x1, n2, m2, r2, qkv, a, aux, x2, t, mc, rc) + bs + (x3,) + ss + (n5, m5, r5, pre2, x5, m6, r6)
    return y, saved


def conformer_block_bwd(dy, x, P, saved, B, N, h, squeeze=False, drops=None):
    """dy [B*N, D] -> (dx, {parameter gradients by the fork's names, float32}); drops: the forward's"""
    drops = _block_drops(drops)
    n1, m1, r1, pre1, x1, n2, m2, r2, qkv, a, aux, x2 = saved[:12]
    cs, x3, ss = saved[12:19], saved[19], saved[20:24]
    n5, m5, r5, pre2, x5, m6, r6 = saved[24:]
    G = {}
    if drops is None:
        d5, G["final_norm.weight"], G["final_norm.bias"] = _ln_bwd(dy, x5, m6, r6, P["final_norm.weight"])
        db5 = d5
    else:
        d5, db5, G["final_norm.weight"], G["final_norm.bias"] = _ln_bwd_drop(dy, x5, m6, r6, P["final_norm.weight"], drops.ffn2, N)
    dn5, g = silu_ffn_bwd(db5, n5, P["ffn2.lin1.weight"], P["ffn2.lin2.weight"], (pre2,), 0.5)
    _put(G, "ffn2.", FFN_NAMES, g)
    if squeeze:
        x4 = torch.empty_like(x3)
        check(lib.htrvt_se_scale_fwd(ptr(x3), ptr(ss[3]), ptr(x4), B, N, x3.shape[1], dt(x3.dtype), stream()), "se_scale_fwd")
    else:
        x4 = x3
    if drops is None or squeeze:
        d4, G["ffn2_norm.weight"], G["ffn2_norm.bias"] = _ln_bwd(dn5, x4, m5, r5, P["ffn2_norm.weight"], dres=d5)
        d3 = d4
        if squeeze:
            d3, g = se_bwd(d4, x3, P["se.fc1.weight"], P["se.fc2.weight"], B, N, ss)
            _put(G, "se.", ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"), g)
        db3 = d3
        if drops is not None and _site_on(drops.conv):
            db3 = residual_dropout(d3, None, N, drops.conv[2], drops.conv[0], drops.conv[1])
    else:
        d3, db3, G["ffn2_norm.weight"], G["ffn2_norm.bias"] = _ln_bwd_drop(dn5, x3, m5, r5, P["ffn2_norm.weight"], drops.conv, N,
                                                                          dres=d5)
    Pc = _sub(P, "conv_module.")
    dt_, gc = _conv_branch_bwd(db3, cs[0], Pc, cs[3:], B, N)
    if drops is None:
        d2, gc["layer_norm.weight"], gc["layer_norm.bias"] = _ln_bwd(dt_, x2, cs[1], cs[2], Pc["layer_norm.weight"], dres=d3)
        db2 = d2
    else:
        d2, db2, gc["layer_norm.weight"], gc["layer_norm.bias"] = _ln_bwd_drop(dt_, x2, cs[1], cs[2], Pc["layer_norm.weight"],
                                                                               drops.attn, N, dres=d3)
    _put(G, "conv_module.", gc.keys(), gc.values())
    G["attn.proj.weight"], G["attn.proj.bias"] = _pw_wgrad(db2, a)
    dqkv = plain_attention_bwd(qkv, a, _pw_dgrad(db2, P["attn.proj.weight"]), aux, B, N, h,
                               drop=drops.probs if drops is not None else None)
    G["attn.qkv.weight"], G["attn.qkv.bias"] = _pw_wgrad(dqkv, n2)
    dn2 = _pw_dgrad(dqkv, P["attn.qkv.weight"])
    if drops is None:
        d1, G["attn_norm.weight"], G["attn_norm.bias"] = _ln_bwd(dn2, x1, m2, r2, P["attn_norm.weight"], dres=d2)
        db1 = d1
    else:
        d1, db1, G["attn_norm.weight"], G["attn_norm.bias"] = _ln_bwd_drop(dn2, x1, m2, r2, P["attn_norm.weight"], drops.ffn1, N,
                                                                           dres=d2)
    dn1, g = silu_ffn_bwd(db1, n1, P["ffn1.lin1.weight"], P["ffn1.lin2.weight"], (pre1,), 0.5)
    _put(G, "ffn1.", FFN_NAMES, g)
    dx, G["ffn1_norm.weight"], G["ffn1_norm.bias"] = _ln_bwd(dn1, x, m1, r1, P["ffn1_norm.weight"], dres=d1)
    return dx, G


def squeeze_block_fwd(x, P, B, N, h, **kw):
    return conformer_block_fwd(x, P, B, N, h, squeeze=True, **kw)


def squeeze_block_bwd(dy, x, P, saved, B, N, h, drops=None):
    return conformer_block_bwd(dy, x, P, saved, B, N, h, squeeze=True, drops=drops)


def squeezeformer_fwd(x, P, B, N0, h, d1, d2, drops=None, save=True, **kw):
    """SqueezeFormerEncoder on x [B*N0, D]: d1 blocks at N0 tokens, Downsample1D, d2 blocks at N0 // 2, Upsample1D back to N0
    plus the skip, out_norm -> (y, saved).  drops: per block (stage1 then stage2) None or a BlockDrop"""
    drops = drops or [None] * (d1 + d2)
    n = N0 // 2 if N0 > 1 else N0
    saved = ()
    for i in range(d1):
        y, s = squeeze_block_fwd(x, _sub(P, f"stage1.{i}."), B, N0, h, drops=drops[i], save=save, **kw)
        saved, x = saved + (x,) + s, y
    skip, x = x, seq_down2_fwd(x, B, N0)
    for i in range(d2):
        y, s = squeeze_block_fwd(x, _sub(P, f"stage2.{i}."), B, n, h, drops=drops[d1 + i], save=save, **kw)
        saved, x = saved + (x,) + s, y
    z = seq_up_add_fwd(x, skip, B, n, N0)
    y, mean, rstd = layernorm_fwd(z, P["out_norm.weight"], P["out_norm.bias"], kw.get("eps", 1e-5), save)
    return y, saved + (z, mean, rstd)


def squeezeformer_bwd(dy, P, saved, B, N0, h, d1, d2, drops=None):
    """dy [B*N0, D] -> (dx, {parameter gradients by the fork's names, float32}); drops: the forward's"""
    drops = drops or [None] * (d1 + d2)
    n = N0 // 2 if N0 > 1 else N0
    L = BLOCK_SAVED + 1
    z, mean, rstd = saved[-3:]
    G = {}
    dz, G["out_norm.weight"], G["out_norm.bias"] = _ln_bwd(dy, z, mean, rstd, P["out_norm.weight"])
    d = seq_up_add_bwd(dz, B, n, N0)
    for i in reversed(range(d2)):
        blk = saved[(d1 + i) * L:(d1 + i + 1) * L]
        d, g = squeeze_block_bwd(d, blk[0], _sub(P, f"stage2.{i}."), blk[1:], B, n, h, drops[d1 + i])
        _put(G, f"stage2.{i}.", g.keys(), g.values())
    d = convert(seq_down2_bwd(d, B, N0), dz.clone(), accumulate=True) if N0 > 1 else d + dz
    for i in reversed(range(d1)):
        blk = saved[i * L:(i + 1) * L]
        d, g = squeeze_block_bwd(d, blk[0], _sub(P, f"stage1.{i}."), blk[1:], B, N0, h, drops[i])
        _put(G, f"stage1.{i}.", g.keys(), g.values())
    return d, G


