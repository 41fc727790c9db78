"""Autograd wrappers over seq_ops for callers that hold their own tensors: the tests and tools/.

The models do not come through here.  The forks run as full drop-ins -- window/, lgp/, sgm/ -- whose engine (engine.py)
and SGM head (sgm/model/sgm_head.py) call the same seq_ops functions directly, so an operator-level test of a wrapper
below exercises the launch sequence the models run.  Wrapped: the window fork's relative-position attention (table
-driven in bfloat16; in float32 ONE dense bias [heads, N, N], table entries inside a window and MASKED outside, into the
batched-GEMM route), the SGM head's single-head cross-attention, the LGP block's window-12 attention, pool + norm
and scaled up-sampling, the macaron forks' GLU + depthwise token convolution + BatchNorm + SiLU, the VAN forks' depthwise
Conv2d (depthwise_conv2d), the Swin fork's 2-D shifted-window attention (window_attention_2d), and the forks' regularisers
as operators: dropout on the attention probabilities (self_attention, relpos_self_attention(dropout_p=...)) and
residual + drop_path(dropout(x)) (residual_dropout); wiring those into the models is not done here.  mask_tokens is the
multi-mask forks' per-sample token masking x * keep + (1 - keep) * mask_token as an operator (csrc/masking.hip), for stems
that do not end in the ResNet's token assembly.  What stays here is wrapper logic: dtype checks, padding a sequence to the length the kernels
run at, and the index bookkeeping (which table entry each (query, key) pair uses), host glue for the CPU tests."""
import torch

from . import seq_ops
from ._lib import lib
from .ops import colsum, dt
from .seq_ops import relpos_workspace_floats  # noqa: F401  (part of this module's surface)

MASKED = -1.0e30      # "outside the window": finite, so an all-masked key tile cannot produce inf - inf in the online softmax


def _need_device(*tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("htrvt_amd.variants needs device tensors on an MI355X (no CPU fallback); the index bookkeeping "
                           "alone is relative_position_index()")


def _drop(dropout_p, seed, device, n=1):
    """(seed, p) for seq_ops, None for p = 0.  seed=None draws the int64 seed(s) on the device from the CUDA default
    generator (no host sync), as the mixer and the SGM head do."""
    p = float(dropout_p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability {p} outside [0, 1)")
    if p == 0.0:
        return None
    if seed is None:
        seed = torch.randint(0, 2 ** 62, (n,), dtype=torch.int64, device=device)
    if seed.dtype != torch.int64 or seed.numel() != n or not seed.is_cuda:
        raise TypeError(f"seed: an int64 device tensor of {n} element(s) expected")
    return seed.contiguous(), p


def relative_position_index(N, num_patches, window_size=0, shift_size=0):
    """(index [N, N] int64 into the bias table, inside [N, N] bool) for queries i / keys j of the ORIGINAL sequence.
    Full attention (HTR_VT.py:27-31,45-46): index = (j - i) + P - 1.  Windowed (Block._attend, :113-154): the sequence is
    zero-padded to Np = a multiple of the window, token t sits at position (t - shift) mod Np of the rolled sequence,
    window = position // ws, slot = position % ws; a pair attends only inside one window and uses the slots' distance.
    The padding tokens are masked as keys (key_padding_mask, :47-56) and dropped as queries (:150-152), so among the N
    real tokens they only move the window boundaries -- which Np in the modulus reproduces."""
    t = torch.arange(N)
    if window_size <= 0:
        return (t[None, :] - t[:, None]) + num_patches - 1, torch.ones(N, N, dtype=torch.bool)
    Np = (N + window_size - 1) // window_size * window_size
    pos = (t - shift_size) % Np
    win, slot = pos // window_size, pos % window_size
    return (slot[None, :] - slot[:, None]) + num_patches - 1, win[None, :] == win[:, None]


def padded_len(N, dtype, head_dim):
    """sequence length the attention kernels run at, the `ld` to build the bias at for biased_self_attention: a multiple
    of 128 where the fused bfloat16 kernels can serve it (the padding keys carry the bias -1e30, the padding queries are
    dropped), else a multiple of 8 (16-byte rows of the GEMMs)"""
    n128 = (N + 127) // 128 * 128
    if dtype == torch.bfloat16 and lib.htrvt_attn_supported(n128, head_dim, dt(dtype)):
        return n128
    return (N + 7) // 8 * 8


class _RelPosBias(torch.autograd.Function):
    """table [(2P-1), heads] float32 (device) -> dense bias [heads, ld, ld]: lookup + window mask forward, per-entry
    gather-sum backward (no atomics)"""

    @staticmethod
    def forward(ctx, table, N, num_patches, window_size, shift_size, ld):
        ctx.geo = (N, num_patches, window_size, shift_size)
        return seq_ops.relpos_bias_fwd(table.contiguous().float(), N, num_patches, window_size, shift_size, ld)

    @staticmethod
    def backward(ctx, dbias):
        return seq_ops.relpos_bias_bwd(dbias.contiguous().float(), *ctx.geo), None, None, None, None, None


def relative_position_bias(table, N, num_patches, window_size=0, shift_size=0, ld=None):
    """dense float32 [heads, ld, ld] score bias from the learned table [(2 P - 1), heads] (ld >= N: the sequence length the
    attention kernels run at, see biased_self_attention; default N).  Differentiable in the table."""
    _need_device(table)
    return _RelPosBias.apply(table, N, num_patches, window_size, shift_size, N if ld is None else ld)


class _BiasedSelfAttention(torch.autograd.Function):
    """qkv [B*N, 3*heads*hd] (the qkv Linear's output) + dense bias [heads, N, N] -> out [B*N, heads*hd]"""

    @staticmethod
    def forward(ctx, qkv, bias, B, N, heads, drop=None):
        qkv, bias = qkv.contiguous(), bias.contiguous().float()
        # the fused dense-bias kernels have no dropout: with it, the unfused route
        ctx.fused = drop is None and bool(lib.htrvt_attn_supported(N, qkv.shape[1] // 3 // heads, dt(qkv.dtype)))
        ctx.drop = drop
        if ctx.fused:
            out, aux = seq_ops.attention_fwd(qkv, B, N, heads, bias=bias)             # aux = lse
        elif drop is None:
            out, aux = seq_ops.attention_unfused_fwd(qkv, B, N, heads, bias=bias)     # aux = P
        else:
            out, aux = seq_ops.attention_unfused_fwd(qkv, B, N, heads, bias=bias, drop=drop)
        ctx.save_for_backward(qkv, bias, out, aux)
        ctx.dims = (B, N, heads)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, bias, out, aux = ctx.saved_tensors
        dout = dout.contiguous().to(qkv.dtype)
        dbias = torch.zeros_like(bias)
        if ctx.fused:
            dqkv = seq_ops.attention_bwd(qkv, out, dout, aux, *ctx.dims, bias=bias, dbias=dbias)
        elif ctx.drop is None:
            dqkv = seq_ops.attention_unfused_bwd(qkv, aux, dout, *ctx.dims, dbias=dbias)
        else:
            dqkv = seq_ops.attention_unfused_bwd(qkv, aux, dout, *ctx.dims, dbias=dbias, drop=ctx.drop)
        return dqkv, dbias, None, None, None, None


def biased_self_attention(qkv, bias, B, N, heads, drop=None):
    """softmax(q k^T * hd^-0.5 + bias) v over qkv [B*N, 3*heads*hd] (layout [B,N,3,heads,hd]); bias [heads, ld, ld] float32
    with ld >= N (see relative_position_bias; columns >= N must hold -1e30).  bfloat16 with hd in {32, 64, 128}: the fused
    kernels, the sequence zero-padded to a multiple of 128 if it is not one (masked keys, dropped queries); otherwise
    (float32 parity path) batched GEMMs + row softmax at a multiple of 8.  Differentiable in qkv and bias.
    drop = (seed, p): dropout on the probabilities, always on the batched-GEMM route; the mask index ((b heads + head) Np +
    q) Np + k is formed at the padded length Np the route runs at."""
    _need_device(qkv)
    D3 = qkv.shape[1]
    hd = D3 // 3 // heads
    Np = padded_len(N, qkv.dtype, hd)
    ld = bias.shape[-1]
    if ld != Np:
        if ld != N:
            raise ValueError(f"bias is [{heads}, {ld}, {ld}]: expected ld = {N} or the padded length {Np}")
        padded = torch.full((heads, Np, Np), MASKED, dtype=torch.float32, device=bias.device)
        padded[:, :N, :N] = bias            # (glue: a strided copy; use relative_position_bias(..., ld=padded_len) to avoid it)
        padded[:, N:, 0] = 0.0
        bias = padded
    extra = () if drop is None else (drop,)
    if Np == N:
        return _BiasedSelfAttention.apply(qkv, bias, B, N, heads, *extra)
    qp = torch.zeros(B, Np, D3, dtype=qkv.dtype, device=qkv.device)
    qp[:, :N] = qkv.view(B, N, D3)
    out = _BiasedSelfAttention.apply(qp.view(B * Np, D3), bias, B, Np, heads, *extra)
    return out.view(B, Np, -1)[:, :N].reshape(B * N, -1)


class _RelPosSelfAttention(torch.autograd.Function):
    """qkv [B*N, 3*heads*hd] bfloat16 + table [(2P-1), heads] float32 -> out [B*N, heads*hd]: the table-driven fused kernels
    (csrc/attn_relpos.hip), any N >= 32 with no padded copy; the table gradient is reduced without atomics"""

    @staticmethod
    def forward(ctx, qkv, table, B, N, heads, num_patches, window, shift, drop=None):
        if table.dtype != torch.float32:
            raise TypeError(f"relative-position table: float32 expected (the parameter as stored), got {table.dtype}")
        qkv, table = qkv.contiguous(), table.contiguous()
        ctx.dims = (B, N, heads, num_patches, window, shift)
        ctx.drop = {} if drop is None else {"drop": drop}
        out, lse = seq_ops.relpos_attention_fwd(qkv, table, *ctx.dims, **ctx.drop)
        ctx.save_for_backward(qkv, table, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, table, out, lse = ctx.saved_tensors
        dtable = torch.zeros_like(table) if ctx.needs_input_grad[1] else None
        dqkv = seq_ops.relpos_attention_bwd(qkv, table, out, dout.contiguous().to(qkv.dtype), lse, *ctx.dims, dtable=dtable,
                                            **ctx.drop)
        return dqkv, dtable, None, None, None, None, None, None, None


def relpos_supported(N, head_dim, dtype, num_patches, window_size=0, shift_size=0):
    """True where the table-driven fused kernels serve the shape (bfloat16, hd in {64, 128}, 32 <= N <= P <= 2048)"""
    return bool(lib.htrvt_attn_relpos_supported(N, head_dim, dt(dtype), num_patches, window_size, shift_size))


def relpos_self_attention(qkv, table, B, N, heads, num_patches, window_size=0, shift_size=0, dropout_p=0.0, seed=None):
    """Attention.forward + Block._attend of the window fork on the qkv Linear's output: softmax(q k^T hd^-0.5 + table
    bias) v with 1-D (shifted) windows, qkv [B*N, 3*heads*hd] (layout [B,N,3,heads,hd]), table [(2P-1), heads] float32.
    bfloat16: the table-driven fused kernels (no dense bias, no padding); float32 (parity path): the dense bias of
    relative_position_bias + batched GEMMs and row softmax (biased_self_attention).  Differentiable in qkv and table.
    dropout_p > 0: attn_drop of the fork, out = (softmax(.) * keep / (1 - p)) v with keep(b, head, q, k) = keep_elem(seed,
    ((b heads + head) L + q) L + k); seed: an int64 device tensor of one element, None: drawn on the device.  The fused
    kernels form the index at L = N; the float32 route runs (and indexes the mask) at L = N rounded up to a multiple of 8,
    so the two routes share a mask for one seed exactly when N is a multiple of 8."""
    _need_device(qkv, table)
    hd = qkv.shape[1] // 3 // heads
    drop = _drop(dropout_p, seed, qkv.device)
    extra = () if drop is None else (drop,)
    if qkv.dtype == torch.bfloat16:
        if not relpos_supported(N, hd, qkv.dtype, num_patches, window_size, shift_size):
            raise ValueError(f"relative-position attention: {lib.htrvt_last_error().decode()}")
        return _RelPosSelfAttention.apply(qkv, table, B, N, heads, num_patches, window_size, shift_size, *extra)
    bias = relative_position_bias(table, N, num_patches, window_size, shift_size, ld=padded_len(N, qkv.dtype, hd))
    return biased_self_attention(qkv, bias, B, N, heads, *extra)


class _SelfAttention(torch.autograd.Function):
    """qkv [B*N, 3*heads*hd] -> out [B*N, heads*hd], plain scores; drop = (seed, p) or None"""

    @staticmethod
    def forward(ctx, qkv, B, N, heads, drop):
        qkv = qkv.contiguous()
        ctx.fused = bool(lib.htrvt_attn_dropout_supported(N, qkv.shape[1] // 3 // heads, dt(qkv.dtype)))
        ctx.dims, ctx.drop = (B, N, heads), drop
        if ctx.fused:
            out, aux = seq_ops.attention_fwd(qkv, B, N, heads, drop=drop)             # aux = lse
        else:
            out, aux = seq_ops.attention_unfused_fwd(qkv, B, N, heads, drop=drop)     # aux = P
        ctx.save_for_backward(qkv, out, aux)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, aux = ctx.saved_tensors
        dout = dout.contiguous().to(qkv.dtype)
        if ctx.fused:
            dqkv = seq_ops.attention_bwd(qkv, out, dout, aux, *ctx.dims, drop=ctx.drop)
        else:
            dqkv = seq_ops.attention_unfused_bwd(qkv, aux, dout, *ctx.dims, drop=ctx.drop)
        return dqkv, None, None, None, None


def self_attention(qkv, B, N, heads, dropout_p=0.0, seed=None):
    """softmax(q k^T * hd^-0.5) v of model_v1's Attention on the qkv Linear's output, with the forks' attn_drop: out =
    (softmax(.) * keep / (1 - p)) v, keep(b, head, q, k) = keep_elem(seed, ((b heads + head) N + q) N + k).  The fused
    kernels where htrvt_attn_dropout_supported says so (bfloat16, hd in {32, 64, 128}, N >= 32), else batched GEMMs + row
    softmax with the same mask (float32; N a multiple of 8 there).  seed: int64 device tensor of one element, None: drawn
    on the device from the CUDA default generator.  The backward regenerates the mask from the seed."""
    _need_device(qkv)
    hd = qkv.shape[1] // 3 // heads
    if not lib.htrvt_attn_dropout_supported(N, hd, dt(qkv.dtype)) and N % 8:
        raise ValueError(f"self_attention: the batched-GEMM route needs N={N} to be a multiple of 8")
    return _SelfAttention.apply(qkv, B, N, heads, _drop(dropout_p, seed, qkv.device))


class _ResidualDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, rows_per_sample, seeds, p, p_path):
        ctx.args = (rows_per_sample, seeds, p, p_path)
        return seq_ops.residual_dropout(x.contiguous(), res.contiguous(), *ctx.args)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        return seq_ops.residual_dropout(dy, None, *ctx.args), dy, None, None, None, None


def residual_dropout(x, res, B, p, p_path, seeds=None):
    """res + drop_path(dropout(x, p), p_path) of a block's residual branch in one pass: x, res [B*N, D] (float32 or
    bfloat16, D a multiple of 4 / 8); element i of x is kept by keep_elem(seeds[0], i), the whole branch of sample b by
    keep_elem(seeds[1], b), kept values are scaled by 1 / (1 - p) / (1 - p_path).  seeds: int64 device tensor of two
    elements, None: drawn on the device.  Differentiable in x and res; the backward regenerates both masks."""
    _need_device(x, res)
    if x.shape != res.shape or x.dtype != res.dtype or x.dim() != 2 or x.shape[0] % B:
        raise ValueError("residual_dropout: x and res [B*N, D] of one dtype expected")
    for q in (p, p_path):
        if not 0.0 <= float(q) < 1.0:
            raise ValueError(f"dropout probability {q} outside [0, 1)")
    if seeds is None and (p > 0 or p_path > 0):
        seeds = torch.randint(0, 2 ** 62, (2,), dtype=torch.int64, device=x.device)
    if seeds is not None and (seeds.dtype != torch.int64 or seeds.numel() != 2 or not seeds.is_cuda):
        raise TypeError("seeds: an int64 device tensor of two elements expected")
    return _ResidualDropout.apply(x, res, x.shape[0] // B, seeds, float(p), float(p_path))


class _MaskTokens(torch.autograd.Function):
    """x [rows, D], keep float32 [N] or [rows], mask_token float32 [D] -> y (seq_ops.mask_tokens_fwd / _bwd)"""

    @staticmethod
    def forward(ctx, x, keep, mask_token):
        ctx.save_for_backward(keep)
        return seq_ops.mask_tokens_fwd(x, keep, mask_token)

    @staticmethod
    def backward(ctx, dy):
        keep, = ctx.saved_tensors
        dx, dtoken = seq_ops.mask_tokens_bwd(dy.contiguous(), keep, ctx.needs_input_grad[2])
        return dx, None, dtoken


def mask_tokens(x, keep, mask_token):
    """The multi-mask forks' x * keep + (1 - keep) * mask_token (model_sgm_mms_attach/model/HTR_VT.py:377) for a keep
    mask of zeros and ones: x [B, N, D] float32 or bfloat16 (D a multiple of 4 / 8); keep [B, N] or [B, N, 1] (one mask
    per sample) or [N] (one for the batch), any dtype, non-zero = keep; mask_token a float32 parameter of D elements
    ([D] or the forks' [1, 1, D]).  Returns y like x.  Differentiable in x (dy where kept, 0 where masked) and in
    mask_token (the sum of dy over the masked tokens, in float32 and a fixed order: two runs agree bitwise)."""
    _need_device(x, keep, mask_token)
    if x.dim() != 3 or x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("mask_tokens: x [B, N, D] float32 or bfloat16 expected")
    B, N, D = x.shape
    if tuple(keep.shape) not in ((N,), (B, N), (B, N, 1)):
        raise ValueError(f"mask_tokens: keep of shape {tuple(keep.shape)}: [{N}], [{B}, {N}] or [{B}, {N}, 1] expected")
    if mask_token.dtype != torch.float32 or mask_token.numel() != D:
        raise ValueError(f"mask_tokens: mask_token: float32 with {D} elements expected")
    if D % (4 if x.dtype == torch.float32 else 8):
        raise ValueError(f"mask_tokens: D = {D} is no multiple of {4 if x.dtype == torch.float32 else 8}")
    k = keep.to(torch.float32).contiguous().view(-1)
    token = mask_token.contiguous().view(D)
    return _MaskTokens.apply(x.contiguous().view(B * N, D), k, token).view(B, N, D)


class _CrossAttention(torch.autograd.Function):
    """SGMHead._cross_attend (sgm_head.py:118-127): out = softmax(Q K^T / sqrt(D)) K, Q [B,L,D], K = V [B,N,D]"""

    @staticmethod
    def forward(ctx, Q, KV):
        Q, KV = Q.contiguous(), KV.contiguous()
        out, P = seq_ops.cross_attention_fwd(Q, KV)
        ctx.save_for_backward(Q, KV, P)
        return out

    @staticmethod
    def backward(ctx, dout):
        Q, KV, P = ctx.saved_tensors
        return seq_ops.cross_attention_bwd(Q, KV, P, dout.contiguous().to(Q.dtype))


def cross_attention(Q, KV):
    """single-head cross-attention of the SGM head: Q [B, L, D] text queries, KV [B, N, D] visual tokens (K = V).
    N and D multiples of 8 (bfloat16) / 4 (float32); any L."""
    _need_device(Q, KV)
    return _CrossAttention.apply(Q, KV)


# ---- model_lgp (model_lgp/model/plg.py): the three operators of LocalGlobalParallelBlockSimple, csrc/lgp.hip ------------

class _LocalWindowAttention(torch.autograd.Function):
    """qkv [B*N, 3*heads*hd] + the qkv Linear's float32 bias [3*heads*hd] -> out [B*N, heads*hd]: WindowMHSA1D between its
    Linear layers.  The bias is an input because the reference's zero padding tokens of a ragged last window become rows
    equal to it, which real queries attend to; its k / v thirds get the gradient of those rows."""

    @staticmethod
    def forward(ctx, qkv, qkv_bias, B, N, heads, window, shift):
        if qkv_bias.dtype != torch.float32:
            raise TypeError(f"qkv bias: float32 expected (the parameter as stored), got {qkv_bias.dtype}")
        qkv, qkv_bias = qkv.contiguous(), qkv_bias.contiguous()
        ctx.save_for_backward(qkv, qkv_bias)
        ctx.dims = (B, N, heads, window, shift)
        return seq_ops.local_attention_fwd(qkv, qkv_bias, *ctx.dims)

    @staticmethod
    def backward(ctx, dout):
        B, N, _, window, _ = ctx.dims
        qkv, qkv_bias = ctx.saved_tensors
        D = qkv.shape[1] // 3
        dqkv, dpad = seq_ops.local_attention_bwd(qkv, qkv_bias, dout.contiguous().to(qkv.dtype), *ctx.dims)
        dbias = None
        if ctx.needs_input_grad[1]:
            dbias = torch.zeros_like(qkv_bias)
            if N % window:
                colsum(dpad, B, 2 * D, 2 * D, dbias.data_ptr() + 4 * D, dti=dt(torch.float32))
        return dqkv, dbias, None, None, None, None, None


def local_attention_supported(head_dim, window, dtype, shift=0):
    return bool(lib.htrvt_attn_local_shift_supported(head_dim, window, shift, dt(dtype)))


def local_window_attention(qkv, qkv_bias, B, N, heads, window, shift=0):
    """WindowMHSA1D of the LGP and SGM local-global forks on its qkv Linear's output: attention inside non-overlapping
    windows of `window` tokens, the padding slots of a ragged last window being rows equal to `qkv_bias` (not masked).
    shift (0 ... window - 1): the windows of the tokens rolled by `shift`, as torch.roll(x, shift, 1) in front of the
    padding and the roll back behind the crop give them; no mask across the wrap.  Differentiable in qkv and the bias."""
    _need_device(qkv, qkv_bias)
    if not local_attention_supported(qkv.shape[1] // 3 // heads, window, qkv.dtype, shift):
        raise ValueError(f"window attention: {lib.htrvt_last_error().decode()}")
    return _LocalWindowAttention.apply(qkv, qkv_bias, B, N, heads, window, shift)


class _PoolNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, B, N, G, eps):
        z, _, rstd = seq_ops.pool_norm_fwd(x.contiguous(), B, N, G, eps)
        ctx.save_for_backward(z, rstd)
        ctx.dims = (B, N, G)
        return z

    @staticmethod
    def backward(ctx, dz):
        z, rstd = ctx.saved_tensors
        return seq_ops.pool_norm_bwd(dz.contiguous().to(z.dtype), z, rstd, *ctx.dims), None, None, None, None


def pool_norm(x, B, N, G, eps=1e-5):
    """PooledGlobalMHSA up to its qkv: adaptive average pooling of x [B*N, D] to G tokens per image, then LayerNorm without
    affine -> [B*G, D]"""
    _need_device(x)
    return _PoolNorm.apply(x, B, N, G, eps)


class _UpsampleScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, logit_alpha, B, G, N):
        if logit_alpha.dtype != torch.float32:
            raise TypeError(f"logit_alpha: float32 expected (the parameter as stored), got {logit_alpha.dtype}")
        y = y.contiguous()
        ctx.save_for_backward(y, logit_alpha)
        ctx.dims = (B, N, G)
        return seq_ops.upsample_fwd(y, logit_alpha, torch.empty(B * N, y.shape[1], dtype=y.dtype, device=y.device), *ctx.dims)

    @staticmethod
    def backward(ctx, dout):
        y, logit_alpha = ctx.saved_tensors
        dalpha = torch.zeros_like(logit_alpha)
        dy = seq_ops.upsample_bwd(dout.contiguous().to(y.dtype), y, logit_alpha, dalpha, *ctx.dims)
        return dy, dalpha, None, None, None


def upsample_scale(y, logit_alpha, B, G, N):
    """the tail of PooledGlobalMHSA: linear interpolation of y [B*G, D] back to N tokens per image (align_corners=False)
    times sigmoid(logit_alpha), logit_alpha a 0-dim float32 device tensor -> [B*N, D]"""
    _need_device(y, logit_alpha)
    return _UpsampleScale.apply(y, logit_alpha, B, G, N)


# ---- macaron forks (model_sgm_macaron/model/HTR_VT.py ConvLocalMixer1D): the mixer between its Linear layers, csrc/mixer.hip

class _GluDwconvBnSilu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, weight, bn_weight, bn_bias, conv_bias, running_mean, running_var, num_batches_tracked, B, N, training,
                eps, momentum):
        u, weight = u.contiguous(), weight.contiguous()
        bn = None if bn_weight is None else (bn_weight.contiguous(), bn_bias.contiguous(), running_mean, running_var,
                                             num_batches_tracked)
        conv_bias = None if conv_bias is None else conv_bias.contiguous()
        s, saved = seq_ops.conv_mixer_fwd(u, weight, B, N, bn=bn, training=training, eps=eps, momentum=momentum,
                                          conv_bias=conv_bias)
        ctx.save_for_backward(u, weight, None if bn is None else bn[0], *saved)
        ctx.dims = (B, N, training)
        return s

    @staticmethod
    def backward(ctx, ds):
        u, weight, gamma, *saved = ctx.saved_tensors
        B, N, training = ctx.dims
        du, dweight, dgamma, dbeta, dbias = seq_ops.conv_mixer_bwd(
            ds.contiguous().to(u.dtype), u, weight, B, N, saved, gamma=gamma, training=training,
            need_bias=gamma is None and ctx.needs_input_grad[4])
        return (du, dweight, dgamma, dbeta, dbias) + (None,) * 8


def glu_dwconv_bn_silu(u, weight, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, B, N, training,
                       eps=1e-5, momentum=0.1, conv_bias=None):
    """ConvLocalMixer1D between pw_in and pw_out: u [B*N, 2*D] (float32 or bfloat16) -> silu(bn(dwconv(glu(u)))) [B*N, D].
    weight: dwconv.weight float32 [D, 1, k], k odd <= 15, zero padding per image.  bn_weight / bn_bias float32 [D] with the
    running buffers (training: batch statistics, the buffers updated in place; else the running statistics), or all None
    for use_bn=False, where conv_bias (float32 [D] or None) is added instead.  D a multiple of 8.  Differentiable in u,
    weight, bn_weight, bn_bias and conv_bias."""
    tensors = [t for t in (u, weight, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, conv_bias)
               if t is not None]
    _need_device(*tensors)
    if any(t.dtype != torch.float32 for t in tensors[1:] if t.is_floating_point()):
        raise TypeError("glu_dwconv_bn_silu: float32 parameters and buffers expected (as stored)")
    if (bn_weight is None) != (running_mean is None) or (bn_weight is not None and conv_bias is not None):
        raise ValueError("glu_dwconv_bn_silu: either BatchNorm (weight, bias, running buffers) or a convolution bias")
    return _GluDwconvBnSilu.apply(u, weight, bn_weight, bn_bias, conv_bias, running_mean, running_var, num_batches_tracked,
                                  B, N, bool(training), float(eps), float(momentum))


# ---- VAN forks (model_sgm_mms_attach_van/model/HTR_VT.py LargeKernelAttention / HorizontalMixer): depthwise Conv2d, csrc/van.hip

class _DepthwiseConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, dilation):
        x, weight = x.contiguous(), weight.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.dilation = dilation
        return seq_ops.dwconv_fwd(x, weight, dilation)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dweight = seq_ops.dwconv_bwd(dy.contiguous().to(x.dtype), x, weight, ctx.dilation)
        return dx, dweight, None


def depthwise_conv2d(x_nhwc, weight, dilation=1):
    """nn.Conv2d(C, C, (kh, kw), padding=((kh // 2) * dilation, (kw // 2) * dilation), dilation=dilation, groups=C,
    bias=False) on x_nhwc [B, H, W, C] (float32 or bfloat16, C a multiple of 8) -> [B, H, W, C].  weight: the Conv2d's
    float32 [C, 1, kh, kw], kh odd <= 7, kw odd <= 9, dilation 1 ... 3; zero padding per image.  Differentiable in x_nhwc and
    weight; the gradients are bitwise reproducible."""
    _need_device(x_nhwc, weight)
    if weight.dtype != torch.float32:
        raise TypeError(f"depthwise_conv2d: float32 weight expected (the parameter as stored), got {weight.dtype}")
    if x_nhwc.dim() != 4 or weight.dim() != 4 or weight.shape[0] != x_nhwc.shape[3] or weight.shape[1] != 1:
        raise ValueError(f"depthwise_conv2d: x [B, H, W, C] and weight [C, 1, kh, kw] expected, got {tuple(x_nhwc.shape)} "
                         f"and {tuple(weight.shape)}")
    return _DepthwiseConv2d.apply(x_nhwc, weight, int(dilation))


# ---- Swin fork (model_sgm_mms_swin/model/HTR_VT.py WindowAttention2D inside SwinBlock2D): 2-D shifted windows, csrc/swin.hip

class _WindowAttention2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, B, H, W, heads, window, shift):
        qkv, table = qkv.contiguous(), table.contiguous()
        ctx.save_for_backward(qkv, table)
        ctx.dims = (B, H, W, heads, window, shift)
        return seq_ops.win2d_attention_fwd(qkv, table, *ctx.dims)

    @staticmethod
    def backward(ctx, dout):
        qkv, table = ctx.saved_tensors
        dtable = torch.zeros_like(table) if ctx.needs_input_grad[1] else None
        dqkv = seq_ops.win2d_attention_bwd(qkv, table, dout.contiguous().to(qkv.dtype), *ctx.dims, dtable=dtable)
        return (dqkv, dtable) + (None,) * 6


def win2d_supported(head_dim, window, dtype):
    return bool(lib.htrvt_attn_win2d_supported(head_dim, window[0], window[1], dt(dtype)))


def window_attention_2d(qkv, table, B, H, W, heads, window, shift=(0, 0)):
    """WindowAttention2D as SwinBlock2D calls it, on its qkv Linear's output: qkv [B*H*W, 3*heads*hd] (float32 or
    bfloat16, hd 32 / 64 / 128) in plain token order -> [B*H*W, heads*hd], attention inside the window = (wh, ww) windows
    (wh * ww <= 32) of the map rolled by -shift, with the bias of table (the float32 parameter [(2wh-1)(2ww-1), heads])
    and the fork's additive -100 mask between the wrapped regions.  Differentiable in qkv and table; the gradients are
    bitwise reproducible."""
    _need_device(qkv, table)
    if table.dtype != torch.float32:
        raise TypeError(f"window_attention_2d: float32 table expected (the parameter as stored), got {table.dtype}")
    window, shift = tuple(int(v) for v in window), tuple(int(v) for v in shift)
    entries = (2 * window[0] - 1) * (2 * window[1] - 1)
    # the kernels see pointers only: a shape that disagrees with (B, H, W, heads, window) would send them past a buffer
    if qkv.dim() != 2 or heads < 1 or qkv.shape[0] != B * H * W or qkv.shape[1] % (3 * heads):
        raise ValueError(f"window_attention_2d: qkv [B*H*W = {B * H * W}, 3*heads*hd] expected for heads = {heads}, got "
                         f"{tuple(qkv.shape)}")
    if tuple(table.shape) != (entries, heads):
        raise ValueError(f"window_attention_2d: table [(2wh-1)(2ww-1) = {entries}, heads = {heads}] expected for window "
                         f"{window}, got {tuple(table.shape)}")
    if not win2d_supported(qkv.shape[1] // 3 // heads, window, qkv.dtype):
        raise ValueError(f"window attention: {lib.htrvt_last_error().decode()}")
    return _WindowAttention2D.apply(qkv, table, B, H, W, heads, window, shift)


# ---- SVTR fork (model_sgm_mms_svtr/model/svtr.py MultiHeadSelfAttention with local=True): 2-D neighbourhood attention,
# csrc/svtr.hip

class _NeighborhoodAttention2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, B, H, W, heads, kernel):
        qkv = qkv.contiguous()
        out, lse = seq_ops.nbr2d_attention_fwd(qkv, B, H, W, heads, kernel, save=True)
        ctx.save_for_backward(qkv, out, lse)
        ctx.dims = (B, H, W, heads, kernel)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        return (seq_ops.nbr2d_attention_bwd(qkv, out, dout.contiguous().to(qkv.dtype), lse, *ctx.dims),) + (None,) * 5


def nbr2d_supported(head_dim, kernel, dtype):
    return bool(lib.htrvt_attn_nbr2d_supported(head_dim, kernel[0], kernel[1], dt(dtype)))


def neighborhood_attention_2d(qkv, B, H, W, heads, kernel=(7, 11)):
    """The attention of the SVTR fork's local MultiHeadSelfAttention, on its qkv Linear's output: qkv [B*H*W, 3*heads*hd]
    (float32 or bfloat16, hd 32 / 64) in plain token order -> [B*H*W, heads*hd].  Query (y, x) of the [H, W] map attends to the
    keys within kernel[0] // 2 rows and kernel[1] // 2 columns of it (kernel odd, at most (7, 11)); keys outside the map do not
    exist.  Differentiable in qkv; the gradient is bitwise reproducible."""
    _need_device(qkv)
    kernel = tuple(int(v) for v in kernel)
    # the kernels see pointers only: a shape that disagrees with (B, H, W, heads) would send them past a buffer
    if qkv.dim() != 2 or heads < 1 or B < 0 or H < 1 or W < 1 or qkv.shape[0] != B * H * W or qkv.shape[1] % (3 * heads):
        raise ValueError(f"neighborhood_attention_2d: qkv [B*H*W = {B * H * W}, 3*heads*hd] expected for heads = {heads}, got "
                         f"{tuple(qkv.shape)}")
    if len(kernel) != 2 or not nbr2d_supported(qkv.shape[1] // 3 // heads, kernel, qkv.dtype):
        raise ValueError(f"neighbourhood attention: {lib.htrvt_last_error().decode()}")
    return _NeighborhoodAttention2D.apply(qkv, B, H, W, heads, kernel)


# ---- convolutional forks (model_sgm_mms_conv*/model/HTR_VT.py ConvModule, SqueezeExcite1D, Downsample1D, Upsample1D): csrc/gnmixer.hip

def _f32_params(name, *params):
    if any(t.dtype != torch.float32 for t in params):
        raise TypeError(f"{name}: float32 parameters expected (as stored)")


class _GluDwconvGnSilu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, weight, bias, gn_weight, gn_bias, B, N, eps):
        u, weight, bias, gn_weight, gn_bias = [t.contiguous() for t in (u, weight, bias, gn_weight, gn_bias)]
        s, saved = seq_ops.gn_mixer_fwd(u, weight, bias, gn_weight, gn_bias, B, N, eps)
        ctx.save_for_backward(u, weight, gn_weight, gn_bias, *saved)
        ctx.dims = (B, N)
        return s

    @staticmethod
    def backward(ctx, ds):
        u, weight, gamma, beta, *saved = ctx.saved_tensors
        grads = seq_ops.gn_mixer_bwd(ds.contiguous().to(u.dtype), u, weight, gamma, beta, *ctx.dims, saved)
        return grads + (None,) * 3


def glu_dwconv_gn_silu(u, weight, bias, gn_weight, gn_bias, B, N, eps=1e-5):
    """ConvModule between its 1x1 convolutions: u [B*N, 2*C] (float32 or bfloat16) -> silu(GroupNorm(1, C)(dwconv(glu(u)) +
    bias)) [B*N, C].  weight: depthwise_conv.weight float32 [C, 1, k], k odd <= 15, zero padding per image; bias, gn_weight,
    gn_bias float32 [C].  The statistics are per image over its C * N values, in train and eval mode alike.  C a multiple of
    8 (bfloat16) or 4.  Differentiable in all five tensors; the gradients are bitwise reproducible."""
    _need_device(u, weight, bias, gn_weight, gn_bias)
    _f32_params("glu_dwconv_gn_silu", weight, bias, gn_weight, gn_bias)
    if u.dim() != 2 or u.shape[0] != B * N or weight.dim() != 3 or u.shape[1] != 2 * weight.shape[0] or weight.shape[1] != 1:
        raise ValueError(f"glu_dwconv_gn_silu: u [B*N, 2*C] and weight [C, 1, k] expected, got {tuple(u.shape)} and "
                         f"{tuple(weight.shape)}")
    return _GluDwconvGnSilu.apply(u, weight, bias, gn_weight, gn_bias, B, N, float(eps))


class _SqueezeExcite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, B, N):
        x, w1, b1, w2, b2 = [t.contiguous() for t in (x, w1, b1, w2, b2)]
        y, saved = seq_ops.se_fwd(x, w1, b1, w2, b2, B, N)
        ctx.save_for_backward(x, w1, w2, *saved)
        ctx.dims = (B, N)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, *saved = ctx.saved_tensors
        dx, g = seq_ops.se_bwd(dy.contiguous().to(x.dtype), x, w1, w2, *ctx.dims, saved)
        return (dx,) + g + (None, None)


def squeeze_excite(x, fc1_w, fc1_b, fc2_w, fc2_b, B, N):
    """SqueezeExcite1D on x [B*N, D] (float32 or bfloat16): x * sigmoid(fc2(silu(fc1(mean over the N tokens of the image)))).
    fc1_w [H, D], fc1_b [H], fc2_w [D, H], fc2_b [D] float32; the MLP runs in float32.  Differentiable in all five."""
    _need_device(x, fc1_w, fc1_b, fc2_w, fc2_b)
    _f32_params("squeeze_excite", fc1_w, fc1_b, fc2_w, fc2_b)
    if x.dim() != 2 or x.shape[0] != B * N or fc1_w.shape[1] != x.shape[1] or tuple(fc2_w.shape) != tuple(fc1_w.shape)[::-1]:
        raise ValueError(f"squeeze_excite: x [B*N, D], fc1_w [H, D], fc2_w [D, H] expected, got {tuple(x.shape)}, "
                         f"{tuple(fc1_w.shape)}, {tuple(fc2_w.shape)}")
    return _SqueezeExcite.apply(x, fc1_w, fc1_b, fc2_w, fc2_b, B, N)


class _SeqDownsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, B, N):
        ctx.dims = (B, N)
        return seq_ops.seq_down2_fwd(x.contiguous(), B, N)

    @staticmethod
    def backward(ctx, dy):
        return seq_ops.seq_down2_bwd(dy.contiguous(), *ctx.dims), None, None


def seq_downsample2(x, B, N):
    """Downsample1D on x [B*N, D]: avg_pool1d(2, 2) along the tokens -> [B*(N // 2), D]; N <= 1 is the identity"""
    _need_device(x)
    if x.dim() != 2 or x.shape[0] != B * N:
        raise ValueError(f"seq_downsample2: x [B*N, D] expected, got {tuple(x.shape)}")
    return x if N <= 1 else _SeqDownsample2.apply(x, B, N)


class _SeqUpsampleAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, skip, B, n, N0):
        ctx.dims = (B, n, N0)
        return seq_ops.seq_up_add_fwd(y.contiguous(), skip.contiguous(), B, n, N0)

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        return seq_ops.seq_up_add_bwd(dout, *ctx.dims), dout, None, None, None


def seq_upsample_add(y, skip, B, n, N0):
    """Upsample1D fused with the skip add: y [B*n, D], skip [B*N0, D] -> skip + y at token (i * n) // N0, F.interpolate's
    nearest index"""
    _need_device(y, skip)
    if y.dim() != 2 or skip.dim() != 2 or y.shape[0] != B * n or skip.shape[0] != B * N0 or y.shape[1] != skip.shape[1] \
            or y.dtype != skip.dtype or not 1 <= n <= N0:
        raise ValueError(f"seq_upsample_add: y [B*n, D] and skip [B*N0, D] of one dtype expected, got {tuple(y.shape)} and "
                         f"{tuple(skip.shape)}")
    return _SeqUpsampleAdd.apply(y, skip, B, n, N0)
