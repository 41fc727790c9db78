"""References, inputs and case lists of the small streaming ("glue") kernels that run in every step: bfloat16 conversions,
column / row sums, token masking, the dense relative-position bias, AdamW / SAM and the float32 element-wise steps.

Written from include/htrvt.h, the comments at the head of each .hip file and the reference model's semantics -- not from the
kernel bodies.  Nothing here needs a GPU: tests/test_glue_refs_cpu.py checks every function against torch's own operators or
float64 autograd and shows that the comparisons of tests/test_glue_kernels_gpu.py reject a list of injected faults; the GPU
file then holds the kernels against these functions through the C ABI.
"""
import math

import numpy as np
import torch

MASKED = -1.0e30
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ------------------------------------------------------------------ bfloat16 rounding
def bf16_edge_values():
    """float32 values, built from bit patterns, at which a float32 -> bfloat16 conversion can go wrong.  The expected
    result is torch's own .to(torch.bfloat16): round to nearest, ties to even, NaN stays NaN."""
    pos = [
        0x3F808000,   # low half 0x8000 over an EVEN upper half: a tie, stays 0x3F80
        0x3F818000,   # ... over an ODD upper half: a tie, goes up to 0x3F82
        0x3FFF8000,   # a tie whose carry runs into the exponent (0x4000)
        0x3F807FFF, 0x3F817FFF,   # just under the tie: down
        0x3F808001, 0x3F818001,   # just over the tie: up
        0x00000000,   # zero (the negative one below)
        0x00000001, 0x00008000, 0x00018000, 0x00012345, 0x007FFFFF,   # float32 subnormals (the last one rounds to the smallest normal)
        0x00800000,   # the smallest normal
        0x7F7FFFFF,   # the largest float32: rounds to infinity
        0x7F7F8000,   # a tie at the top of the range: infinity as well
        0x7F7F7FFF,   # the largest value that stays finite
        0x7F800000,   # infinity
    ]
    bits = pos + [b | 0x80000000 for b in pos] + [0x7FC00000]      # both signs, then a quiet NaN
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def with_edges(shape, seed):
    """float32 [shape]: random real values over six decades (randn * logspace(-3, 3) along the last axis) with
    bf16_edge_values() tiled over every 7th element of the flattened tensor, so that the edges meet every lane position"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * torch.logspace(-3, 3, shape[-1])
    flat = x.reshape(-1)
    e = bf16_edge_values()
    at = torch.arange(0, flat.numel(), 7)
    flat[at] = e[torch.arange(at.numel()) % e.numel()]
    if flat.numel() >= e.numel():           # and once back to back, so that pairs / vectors of edges are converted together
        flat[:e.numel()] = e
    return flat.view(*shape)


def bf16_mismatch(got, src):
    """number of elements of the bfloat16 tensor `got` that are not torch's rounding of the float32 tensor `src`: compared
    as int16 bits (so -0 is not +0 and an off-by-one-ulp is seen), NaN compared as "is NaN".  0 = equal."""
    assert got.dtype == BF and src.dtype == F32 and got.shape == src.shape, (got.dtype, src.dtype, got.shape, src.shape)
    want = src.cpu().to(BF)
    got = got.cpu()
    nan_w, nan_g = torch.isnan(want), torch.isnan(got)
    bad = (nan_w != nan_g) | (~nan_w & (got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)))
    return int(bad.sum())


def bits_mismatch(got, want):
    """number of elements of two same-typed tensors / arrays that differ as bit patterns, NaN compared as "is NaN" """
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    want = want.detach().cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    nan_w, nan_g = torch.isnan(want), torch.isnan(got)
    bad = (nan_w != nan_g) | (~nan_w & (got.contiguous().view(ints) != want.contiguous().view(ints)))
    return int(bad.sum())


def split_bf16_ref(x):
    """hi = bf16(x), lo = bf16(x - hi) (include/htrvt.h); hi infinite (x infinite or beyond bfloat16's range): lo = 0, so that
    hi + lo stays infinite instead of inf - inf (csrc/split.hip's head comment)"""
    hi = x.to(BF)
    d = torch.where(torch.isinf(hi.float()), torch.zeros_like(x), x - hi.float())
    return hi, d.to(BF)


# ------------------------------------------------------------------ column / row sums
def colsum_ref(x, rows, cols, ld, keep=None, keep_mod=1):
    """sum over the rows of columns [0, cols) of the [rows][ld] array at the start of `x` (any shape, taken flat), in the
    dtype of x.  With `keep` (float [>= keep_mod]) only the rows with keep[r % keep_mod] == 0 count -- the MASKED rows, the
    rule of the mask-token gradient; without it every row."""
    flat = x.reshape(-1)
    assert flat.numel() >= (rows - 1) * ld + cols       # the last row needs its `cols` columns only
    a = flat.as_strided((rows, cols), (ld, 1))
    if keep is not None:
        sel = keep.reshape(-1).cpu()[torch.arange(rows) % keep_mod] == 0
        a = a[sel.to(a.device)]
    return a.sum(0)


def colsum_splits(rows):
    """row splits of htrvt_colsum as htrvt_colsum_workspace_floats documents them: one below 256 rows, then rows // 128, at
    most 64"""
    return 1 if rows < 256 else min(rows // 128, 64)


def rowsum_f32_ref(partial, out):
    """numpy float32: the rows of partial [rows][cols] added one by one in ascending order, then out + that sum -- the order
    htrvt_rowsum_f32 documents"""
    partial = np.asarray(partial, dtype=np.float32)
    a = np.zeros(partial.shape[1], dtype=np.float32)
    for r in range(partial.shape[0]):
        a = a + partial[r]
    return np.asarray(out, dtype=np.float32) + a


# ------------------------------------------------------------------ token masking
def mask_tokens_fwd_ref(x, keep, keep_mod, token):
    """y[r] = x[r] where keep[r % keep_mod] != 0, else the token (rounded to x's dtype); torch.where: nothing of a masked
    row's x reaches y"""
    rows = x.shape[0]
    k = (keep.reshape(-1)[torch.arange(rows) % keep_mod] != 0)[:, None]
    return torch.where(k, x, token.to(x.dtype)[None, :].expand_as(x))


def mask_tokens_bwd_ref(dy, keep, keep_mod):
    rows = dy.shape[0]
    k = (keep.reshape(-1)[torch.arange(rows) % keep_mod] != 0)[:, None]
    return torch.where(k, dy, torch.zeros_like(dy))


# ------------------------------------------------------------------ dense relative-position bias
def window_layout(N, P, ws, shift, _roll_sign=-1):
    """(window [N], slot [N]) of every real token, read off the windows the reference model builds (Block._attend): pad the
    token numbers to a multiple of the window, roll them by -shift, cut into rows of ws.  ws <= 0: one window, slot = token.
    A window wider than num_patches is refused as the reference's Attention.forward refuses it (its windows are sequences of
    ws tokens, longer than the table serves)."""
    if N > P:
        raise ValueError(f"N={N} exceeds num_patches={P}")
    if ws <= 0:
        return torch.zeros(N, dtype=torch.long), torch.arange(N)
    if ws > P:
        raise ValueError(f"window {ws} exceeds num_patches={P}")
    Np = (N + ws - 1) // ws * ws
    tok = torch.arange(Np)                      # numbers >= N are the zero padding
    if shift > 0:
        tok = torch.roll(tok, _roll_sign * shift)
    wins = tok.view(-1, ws)
    win, slot = torch.full((N,), -1, dtype=torch.long), torch.full((N,), -1, dtype=torch.long)
    for w in range(wins.shape[0]):
        for s in range(ws):
            t = int(wins[w, s])
            if t < N:
                win[t], slot[t] = w, s
    assert (win >= 0).all()
    return win, slot


def relpos_bias_ref(table, N, P, ws, shift, ld, _roll_sign=-1):
    """table [(2P-1)][heads] -> bias [heads][ld][ld]: table[slot_j - slot_i + P - 1][h] where tokens i and j share a window,
    -1e30 elsewhere and in the columns j >= N; the padding rows i >= N are [0, -1e30, ...]"""
    win, slot = window_layout(N, P, ws, shift, _roll_sign)
    heads = table.shape[1]
    idx = slot[None, :] - slot[:, None] + P - 1
    inside = win[None, :] == win[:, None]
    bias = torch.full((heads, ld, ld), MASKED, dtype=table.dtype)
    safe = torch.where(inside, idx, torch.zeros_like(idx))
    bias[:, :N, :N] = torch.where(inside[None], table[safe].permute(2, 0, 1), torch.full((), MASKED, dtype=table.dtype))
    bias[:, N:, 0] = 0.0
    return bias


def relpos_attending(N, P, ws, shift):
    """inside [N][N] bool: the pairs that attend"""
    win, _ = window_layout(N, P, ws, shift)
    return win[None, :] == win[:, None]


def relpos_bias_bwd_ref(dbias, N, P, ws, shift, ld):
    """dbias [heads][ld][ld] -> dtable [(2P-1)][heads]: per entry the sum of dbias over the attending pairs that use it (only
    those elements are read, whatever the others hold); an entry no pair uses is 0"""
    win, slot = window_layout(N, P, ws, shift)
    heads = dbias.shape[0]
    idx = slot[None, :] - slot[:, None] + P - 1
    inside = win[None, :] == win[:, None]
    dtable = torch.zeros(2 * P - 1, heads, dtype=dbias.dtype)
    dtable.index_put_((idx[inside],), dbias[:, :N, :N][:, inside].t().contiguous(), accumulate=True)
    return dtable


# ------------------------------------------------------------------ AdamW, SAM
def adamw_scalars_ref(lr, b1, b2, eps, wd, step):
    """the seven derived scalars of include/htrvt.h, formed in Python doubles and rounded once, and the zero pad"""
    bc1 = 1.0 - math.pow(b1, float(step))
    bc2s = math.sqrt(1.0 - math.pow(b2, float(step)))
    return np.array([1.0 - lr * wd, 1.0 - b1, b2, 1.0 - b2, eps, bc2s, -(lr / bc1), 0.0], dtype=np.float64).astype(np.float32)


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, scalars=None, _fma_v=False):
    """one step of torch's single-tensor AdamW in numpy float32, one rounding per operation, in its statement order:
    p *= 1 - lr wd; m += (1 - b1)(g - m); v = v b2 + ((1 - b2) g) g; denom = sqrt(v) / sqrt(bc2) + eps;
    p += (-(lr / bc1) m) / denom.  -> (p, m, v), new arrays"""
    s = adamw_scalars_ref(lr, b1, b2, eps, wd, step) if scalars is None else np.asarray(scalars, dtype=np.float32)
    decay, w1, b2f, w2, epsf, bc2s, neg = (np.float32(x) for x in s[:7])
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    p = p * decay
    m = m + w1 * (g - m)
    if _fma_v:      # the injected fault: the product (w2 g) g kept exact into the sum, one rounding instead of two
        v = ((v * b2f).astype(np.float64) + (w2 * g).astype(np.float64) * g.astype(np.float64)).astype(np.float32)
    else:
        v = v * b2f + (w2 * g) * g
    denom = np.sqrt(v) / bc2s + epsf
    p = p + (neg * m) / denom
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def sam_scale_ref(norm_sq, rho):
    """rho / (|g| + 1e-12) as torch evaluates `float / tensor` on float32: reciprocal, then multiply (utils/sam.py:20-21)"""
    n = np.sqrt(np.float32(norm_sq)) + np.float32(1e-12)
    return np.float32(1.0) / n * np.float32(rho)


def sam_climb_ref(p, g, norm_sq, rho):
    """p + g * scale in numpy float32, product rounded, then the sum"""
    return np.asarray(p, dtype=np.float32) + np.asarray(g, dtype=np.float32) * sam_scale_ref(norm_sq, rho)


# ------------------------------------------------------------------ float32 element-wise steps
def gelu_ref(x):
    """exact-erf GELU (timm Mlp, HTR_VT.py:76) in the dtype of x"""
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad_mul_ref(a, b):
    """a * gelu'(b), gelu'(b) = Phi(b) + b phi(b)"""
    return a * (0.5 * (1.0 + torch.erf(b * (1.0 / math.sqrt(2.0)))) + b * torch.exp(-0.5 * b * b) * (1.0 / math.sqrt(2.0 * math.pi)))


def elementwise_inputs(n, seed):
    """randn * 2 plus a ramp over [-9, 9]: the tails of erf and of the Gaussian are visited"""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(-9.0, 9.0, n)
    return torch.randn(n, generator=g) * 2 + ramp, torch.randn(n, generator=g) * 2 + ramp.flip(0)


# ------------------------------------------------------------------ case lists, shared by the CPU and the GPU file
CAST_BLOCK_CAP, CAST_THREADS = 2048, 256                    # grid_for in csrc/bwd.hip
CAST_N = [1, 255, 257, CAST_BLOCK_CAP * CAST_THREADS + 3]
CAST_TRANSPOSE_CASES = [(1, 1, 8), (63, 65, 64), (64, 64, 64), (65, 63, 72), (130, 70, 136), (60, 70, 72)]
PACK_CASES = [(5, 3, 1), (33, 65, 4), (37, 21, 9), (64, 32, 9)]

COLSUM_ROWS = [1, 31, 33, 127, 128, 255, 256, 257, 8191, 8192, 8193, 12345]
COLSUM_COLS = {BF: [8, 248, 256, 264], F32: [4, 124, 128, 132]}


def colsum_cases(dtype):
    """(rows, cols, ld): row count number i runs at the widths number i % 4 and (i + 1) % 4, so every row count meets two
    widths and every width six row counts; ld = cols at the first of the two widths and cols + 16 at the second, so every row
    count and every width runs dense and padded."""
    W = COLSUM_COLS[dtype]
    out = []
    for i, rows in enumerate(COLSUM_ROWS):
        for k in range(2):
            cols = W[(i + k) % 4]
            out.append((rows, cols, cols + 16 * k))
    return out


COLSUM_FILTER_ROWS = [257, 8193]
COLSUM_REAL = {BF: (12345, 264), F32: (12345, 132)}
ROWSUM_ROWS, ROWSUM_COLS = [1, 7, 8, 9, 17, 64], [1, 63, 64, 65, 200]

MASK_BLOCK_CAP = 8192
MASK_SMALL = {BF: [(1, 1, 8), (5, 7, 24), (4, 33, 264)], F32: [(1, 1, 4), (5, 7, 12), (4, 33, 264)]}       # (B, N, D)
MASK_BIG = (MASK_BLOCK_CAP * 256 + 5, 4)                    # float32 rows, D: one vector per row, past the block cap

# (N, P, ws, shift, ld, heads)
RELPOS_CASES = [
    (33, 33, 0, 0, 33, 1),
    (33, 50, 0, 0, 40, 3),
    (100, 100, 12, 0, 100, 2),
    (100, 128, 12, 11, 128, 2),
    (37, 37, 1, 0, 40, 1),
    (20, 20, 32, 5, 24, 2),       # a window wider than the sequence AND than num_patches: outside the table, must be refused
    (20, 32, 32, 5, 24, 2),       # a window wider than the sequence that the table serves
    (300, 300, 16, 8, 304, 2),    # past the 256-thread loops
    (300, 321, 0, 0, 384, 1),
]


def relpos_in_contract(case):
    N, P, ws, shift, ld, heads = case
    return ws <= P


ADAMW_N = [4, 1020, 2048 * 256 * 4 + 12]
ADAMW_WD = [0.5, 0.0]
ADAMW_HYPER = dict(lr=1e-3, b1=0.9, b2=0.99, eps=1e-8)
SAM_N = [4, 1028, 2048 * 256 * 4 + 12]
ELEMENTWISE_N = [4, 1020, 1028, 768000]


def adamw_inputs(n, seed):
    """p0 and three fresh gradients whose scale varies over 1e-6 .. 1 from element to element (log-uniform, the same in every
    step, so that both terms of every moment update matter: a contraction there shows) and by 1 / 0.1 / 10 from step to step.
    The first has exact zeros in every third element (v stays 0 there, so denom = eps), the last in another third (m and v
    decay alone)."""
    g = torch.Generator().manual_seed(seed)
    p0 = (torch.randn(n, generator=g) * 0.05).numpy()
    decade = 10.0 ** (-6.0 * torch.rand(n, generator=g))
    grads = []
    for k, scale in enumerate((1.0, 0.1, 10.0)):
        gr = torch.randn(n, generator=g) * decade * scale
        if k == 0:
            gr[::3] = 0.0
        if k == 2:
            gr[1::3] = 0.0
        grads.append(gr.numpy())
    return p0, grads
