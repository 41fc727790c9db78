"""The per-step glue kernels through the C ABI (lib.htrvt_*), at their edges, against tests/glue_refs.py:

  htrvt_cast_f32, htrvt_cast_transpose_f32, htrvt_pack_conv_weight(_slots), htrvt_split_bf16     bfloat16 rounding, bit for bit
  htrvt_colsum, htrvt_colsum_workspace_floats, htrvt_rowsum_f32                                   split / block edges, filters
  htrvt_mask_tokens_fwd / _bwd                                                                    small shapes, past the block cap
  htrvt_relpos_bias_fwd / _bwd                                                                    padding, P > N, ragged windows
  htrvt_adamw, htrvt_adamw_dev, htrvt_sumsq, htrvt_sam_first_step, htrvt_sam_restore              past the block cap, bit for bit
  htrvt_elementwise_f32                                                                           per element against float64

Every output lies in a guarded buffer (attn_refs.guarded); the guards are compared after every test.  Conversions are held
against torch's own float32 -> bfloat16 rounding as int16 bits on glue_refs.bf16_edge_values() tiled into random real data
(ties over even and odd, subnormals, the largest float32, infinities, NaN as "is NaN"); sums over integer data, the optimizer
and SAM are bit for bit against numpy float32 restatements with one rounding per operation; no tolerance anywhere there.
The argument checks are exercised in tests/test_glue_refs_cpu.py, never here -- with one exception: the issue's window case
(N, P, ws, shift) = (20, 20, 32, 5) names a window wider than num_patches.  Slots of one window are then up to 31 apart while
the table has the entries -19 .. 19: the forward kernel read table rows -12 .. -1, in front of the buffer.  The reference
model raises for such a window; htrvt_relpos_bias_* now refuses it before any launch, the case stays in the list and this
file asserts the refusal and that nothing was written; (20, 32, 32, 5) is the window wider than the sequence that is served.

Gated (non-exact) outputs: per element against float64, gate = 8 * E32 relative to max |ref| (kernel_refs.gate_check), E32 =
kernel_refs.e32 = the float32 evaluation error of the reference on these very inputs; nothing in a gate comes from the
kernel.  Mode 1 of htrvt_elementwise_f32 uses __expf and fits the plain gate (no extra term was needed).  At n = 4 E32 is the
error of one element and can be arbitrarily small: those inputs are redrawn while E32 < 2^-26 (the rule of
tests/test_dropnorm_gpu.py for its one-row statistics; it reads the reference alone).  Every gated
comparison prints E32, gate, observed and observed / gate (`pytest -s`).  Measured on an MI355X, worst over the cases:

  output                              E32 (range)          worst observed   worst observed / gate
  colsum 12345 x 264  bfloat16        1.5e-7               4.3e-7           0.36
  colsum 12345 x 132  float32         1.3e-7               2.8e-7           0.27
  elementwise mode 0, gelu(a)         1.7e-8 .. 3.0e-8     3.0e-8           0.12
  elementwise mode 1, a * gelu'(b)    1.6e-8 .. 9.6e-8     9.6e-8           0.12
  (the element-wise worst cases sit where the kernel's float32 value IS torch's float32 value of the reference: observed = E32)
Everything else in this file is bit-exact and passed as such, htrvt_adamw / htrvt_adamw_dev included (no contraction, no
approximate square root or division: 2097164 elements, three steps, every bit of p, m and v).
"""
import ctypes

import numpy as np
import pytest
import torch

import attn_refs as AR
import glue_refs as G
import kernel_refs as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS32 = 2.0 ** -24
NAN = float("nan")


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import dt, ptr, stream
    return lib, check, ptr, stream, dt


@pytest.fixture(autouse=True)
def _guards():
    AR._live.clear()
    yield
    if AR._live:
        AR.assert_guards_intact()


def _guarded_copy(t):
    """`t` (host or device) copied into a guarded device buffer"""
    g = AR.guarded(tuple(t.shape), t.dtype, fill=0.0)
    g.copy_(t)
    return g


def _gate(name, got, ref, err):
    ok, obs = R.gate_check(name, got.detach().cpu(), ref, err, False)
    print(f"    {name}: observed / gate {obs / max(8 * err, 1e-300):.2f}")
    assert ok, f"{name}: observed {obs:.3e} of max|ref| is outside 8 * E32 = {8 * err:.3e}"


def _zero_bits(t):
    """every element is +0 (as bits)"""
    ints = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return bool((t.contiguous().view(ints) == 0).all())


# ==========================================================================================================================
# bfloat16 conversions
# ==========================================================================================================================
@pytest.mark.parametrize("n", G.CAST_N)
def test_cast_f32_rounds_like_torch(n):
    lib, check, ptr, stream, dt = _lib()
    src = G.with_edges((n,), n)
    src_d = src.cuda()
    dst = AR.guarded((n,), BF)
    check(lib.htrvt_cast_f32(ptr(src_d), ptr(dst), n, dt(BF), stream()), "cast_f32")
    assert G.bf16_mismatch(dst, src) == 0


@pytest.mark.parametrize("with_dst", [True, False])
@pytest.mark.parametrize("rows,cols,ld_t", G.CAST_TRANSPOSE_CASES)
def test_cast_transpose_f32_rounds_like_torch_and_zero_fills(rows, cols, ld_t, with_dst):
    lib, check, ptr, stream, dt = _lib()
    src = G.with_edges((rows, cols), rows * 1000 + cols)
    src_d = src.cuda()
    dst = AR.guarded((rows, cols), BF) if with_dst else None
    dst_t = AR.guarded((cols, ld_t), BF)
    check(lib.htrvt_cast_transpose_f32(ptr(src_d), ptr(dst), ptr(dst_t), rows, cols, ld_t, dt(BF), stream()), "cast_transpose_f32")
    if with_dst:
        assert G.bf16_mismatch(dst, src) == 0
    assert G.bf16_mismatch(dst_t[:, :rows].contiguous(), src.t().contiguous()) == 0
    assert _zero_bits(dst_t[:, rows:])


def _pads(extent, odd):
    """smallest pad >= extent of the wanted parity: even takes the paired stores, odd the single ones"""
    return extent + ((extent % 2 == 0) if odd else (extent % 2))


def _same_as_source(got, want_f32):
    """a pack output against the float32 source values: torch's rounding for bfloat16, the very bits for float32"""
    return G.bf16_mismatch(got.contiguous(), want_f32.contiguous()) if got.dtype == BF else G.bits_mismatch(got.contiguous(), want_f32.contiguous())


@pytest.mark.parametrize("which", ["fwd", "dgrad", "both"])
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("Co,Ci,taps", G.PACK_CASES)
def test_pack_conv_weight_rounds_like_torch(Co, Ci, taps, dtype, odd, which):
    lib, check, ptr, stream, dt = _lib()
    w = G.with_edges((Co, Ci, taps), Co * 100 + Ci)
    w_d = w.cuda()
    cpi, cpo = _pads(Ci, odd), _pads(Co, odd)
    fwd = AR.guarded((Co, taps, cpi), dtype, fill=0.0) if which != "dgrad" else None
    dgr = AR.guarded((Ci, taps, cpo), dtype, fill=0.0) if which != "fwd" else None
    check(lib.htrvt_pack_conv_weight(ptr(w_d), ptr(fwd), ptr(dgr), Co, Ci, taps, cpi, cpo, dt(dtype), stream()), "pack_conv_weight")
    if fwd is not None:
        assert _same_as_source(fwd[:, :, :Ci].cpu(), w.permute(0, 2, 1)) == 0
        assert _zero_bits(fwd[:, :, Ci:])
    if dgr is not None:
        assert _same_as_source(dgr[:, :, :Co].cpu(), w.permute(1, 2, 0)) == 0
        assert _zero_bits(dgr[:, :, Co:])


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_pack_conv_weight_slots_leaves_the_other_slot_alone(dtype, odd):
    """a 9-tap weight at tap0 = 0 and a 1-tap weight at tap0 = taps of rows that hold taps + 1 taps: each call writes its
    own slots only (the other one holds a canary), the forward pack is the plain one"""
    lib, check, ptr, stream, dt = _lib()
    Co, Ci, taps = 37, 21, 9
    w9, w1 = G.with_edges((Co, Ci, taps), 91), G.with_edges((Co, Ci, 1), 92)
    w9_d, w1_d = w9.cuda(), w1.cuda()
    cpi, cpo = _pads(Ci, odd), _pads(Co, odd)
    for w, w_d, t, tap0 in ((w9, w9_d, taps, 0), (w1, w1_d, 1, taps)):
        joint = AR.guarded((Ci, taps + 1, cpo), dtype, fill=7.0)
        fwd = AR.guarded((Co, t, cpi), dtype, fill=0.0)
        check(lib.htrvt_pack_conv_weight_slots(ptr(w_d), ptr(fwd), ptr(joint), Co, Ci, t, cpi, cpo, taps + 1, tap0, dt(dtype),
                                               stream()), "pack_conv_weight_slots")
        assert _same_as_source(joint[:, tap0:tap0 + t, :Co].cpu(), w.permute(1, 2, 0)) == 0
        other = torch.ones(taps + 1, dtype=torch.bool)
        other[tap0:tap0 + t] = False
        assert bool((joint.cpu()[:, other, :] == 7).all())
        assert _same_as_source(fwd[:, :, :Ci].cpu(), w.permute(0, 2, 1)) == 0 and _zero_bits(fwd[:, :, Ci:])


@pytest.mark.parametrize("rows,cols", [(37, 24), (5, 9)])
def test_split_bf16_every_route_gives_the_same_bits(rows, cols):
    """dense source, ld_src > cols with ld_src % 4 == 0 (still the vector kernel), ld_src % 4 != 0 and a source 4 bytes off
    the 16-byte grid (both the any-shape kernel): all forms of all routes equal glue_refs.split_bf16_ref, hence each other"""
    lib, check, ptr, stream, dt = _lib()
    x = G.with_edges((rows, cols), rows + cols)
    hi, lo = G.split_bf16_ref(x)
    normal = torch.isfinite(x) & (x.abs() >= 2.0 ** -126) & torch.isfinite(hi.float())
    d = (hi.double() + lo.double() - x.double()).abs()
    assert bool((d[normal] <= 2.0 ** -16 * x.double().abs()[normal]).all())

    routes = {}
    routes["dense"] = (x.cuda(), 0, cols)
    wide = torch.full((rows, cols + 4), NAN)
    wide[:, :cols] = x
    routes["ld % 4 == 0"] = (wide.cuda(), 0, cols + 4)
    odd = torch.full((rows, cols + 1), NAN)
    odd[:, :cols] = x
    routes["ld % 4 != 0"] = (odd.cuda(), 0, cols + 1)
    off = torch.full((rows * cols + 4,), NAN)
    off[1:1 + rows * cols] = x.reshape(-1)
    routes["offset 4 bytes"] = (off.cuda(), 4, cols)
    seen = {}
    for name, (buf, byte_off, ld) in routes.items():
        assert buf.data_ptr() % 16 == 0
        src = buf.data_ptr() + byte_off
        for order, parts in ((0, (hi, lo, hi)), (1, (hi, hi, lo))):
            want = torch.cat(parts, dim=1)
            cat = AR.guarded((rows, 3 * cols), BF)
            check(lib.htrvt_split_bf16(src, rows, cols, ld, ptr(cat), order, 0, 0, None, None, stream()), name)
            assert G.bits_mismatch(cat, want) == 0, (name, order)
            catf = AR.guarded((rows, 3 * cols), F32)
            check(lib.htrvt_split_bf16(src, rows, cols, ld, ptr(catf), order, 1, 0, None, None, stream()), name)
            assert G.bits_mismatch(catf, want.float()) == 0, (name, order)
            catt = AR.guarded((cols, 3 * rows), BF)
            check(lib.htrvt_split_bf16(src, rows, cols, ld, ptr(catt), order, 0, 1, None, None, stream()), name)
            assert G.bits_mismatch(catt, torch.cat([p.t() for p in parts], dim=1).contiguous()) == 0, (name, order)
            key = cat.cpu().view(torch.int16)
            assert torch.equal(seen.setdefault(order, key), key), (name, order)
        if cols % 8 == 0 and ld % 4 == 0 and byte_off == 0:        # the planes are served by the vector kernel only
            h2, l2 = AR.guarded((rows, cols), BF), AR.guarded((rows, cols), BF)
            check(lib.htrvt_split_bf16(src, rows, cols, ld, None, 0, 0, 0, ptr(h2), ptr(l2), stream()), name)
            assert G.bits_mismatch(h2, hi) == 0 and G.bits_mismatch(l2, lo) == 0, name


# ==========================================================================================================================
# column sums
# ==========================================================================================================================
def _colsum(lib, check, stream, x_addr, rows, cols, ld, out, keep, keep_mod, dti):
    """htrvt_colsum with a guarded workspace of exactly htrvt_colsum_workspace_floats(rows, cols) floats"""
    nws = lib.htrvt_colsum_workspace_floats(rows, cols)
    assert nws == (0 if rows < 256 else min(rows // 128, 64) * cols)
    ws = AR.guarded((nws,), F32) if nws else None
    check(lib.htrvt_colsum(x_addr, rows, cols, ld, out.data_ptr(), keep.data_ptr() if keep is not None else None, keep_mod, dti,
                           ws.data_ptr() if nws else None, stream()), "colsum")
    return ws


def _int_rows(rows, cols, ld, dtype, seed):
    """integers in [-3, 3] in the columns that count, NaN in the pad columns (which must not be read)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), NAN)
    x[:, :cols] = torch.randint(-3, 4, (rows, cols), generator=g).float()
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_colsum_at_every_split_and_block_edge(dtype):
    """glue_refs.colsum_cases: every row count of the split edges at two widths, every width around the 32-chunk column block
    at six row counts, dense and padded rows.  Integer data: every summation order is exact."""
    lib, check, ptr, stream, dt = _lib()
    for rows, cols, ld in G.colsum_cases(dtype):
        x = _int_rows(rows, cols, ld, dtype, rows + cols)
        x_d = x.cuda()
        want = 5.0 + G.colsum_ref(x.float(), rows, cols, ld)
        out = AR.guarded((cols,), F32, fill=5.0)
        _colsum(lib, check, stream, x_d.data_ptr(), rows, cols, ld, out, None, 1, dt(dtype))
        assert torch.equal(out.cpu(), want), (rows, cols, ld)
        out2 = AR.guarded((cols,), F32, fill=5.0)
        _colsum(lib, check, stream, x_d.data_ptr(), rows, cols, ld, out2, None, 1, dt(dtype))
        assert G.bits_mismatch(out2, out) == 0, (rows, cols, ld)
        AR.assert_guards_intact()


@pytest.mark.parametrize("rows", G.COLSUM_FILTER_ROWS)
@pytest.mark.parametrize("dtype", [BF, F32])
def test_colsum_row_filters(dtype, rows):
    """keep_mod = 16 (divides neither row count: the contract needs r % keep_mod only), keep_mod = rows (the per-sample
    mask), all ones (nothing is summed), all zeros (everything)"""
    lib, check, ptr, stream, dt = _lib()
    cols = G.COLSUM_COLS[dtype][-1]
    x = _int_rows(rows, cols, cols, dtype, rows)
    x_d = x.cuda()
    g = torch.Generator().manual_seed(rows)
    per_row = (torch.rand(rows, generator=g) > 0.4).float()
    per_row[::5] = 0.5
    per_row[1::7] = -0.0
    filters = {"mod 16": ((torch.arange(16) % 3 != 0).float(), 16), "mod rows": (per_row, rows),
               "all ones": (torch.ones(rows), rows), "all zeros": (torch.zeros(16), 16)}
    for name, (keep, keep_mod) in filters.items():
        keep_d = keep.cuda()
        out = AR.guarded((cols,), F32, fill=5.0)
        _colsum(lib, check, stream, x_d.data_ptr(), rows, cols, cols, out, keep_d, keep_mod, dt(dtype))
        want = 5.0 + G.colsum_ref(x.float(), rows, cols, cols, keep, keep_mod)
        assert torch.equal(out.cpu(), want), name
        if name == "all ones":
            assert bool((out.cpu() == 5).all())
        if name == "all zeros":
            assert torch.equal(out.cpu(), 5.0 + G.colsum_ref(x.float(), rows, cols, cols))


@pytest.mark.parametrize("nblk", [9, 300])
def test_colsum_from_a_raw_address_inside_wider_rows(nblk):
    """x = base + 4 D bytes into a float32 [nblk][2 D] array with ld = 2 D, as seq_ops.layernorm_bwd sums dbeta"""
    lib, check, ptr, stream, dt = _lib()
    D = 132
    g = torch.Generator().manual_seed(nblk)
    part = torch.randint(-3, 4, (nblk, 2, D), generator=g).float()
    part_d = part.cuda()
    out = AR.guarded((D,), F32, fill=5.0)
    _colsum(lib, check, stream, part_d.data_ptr() + 4 * D, nblk, D, 2 * D, out, None, 1, dt(F32))
    assert torch.equal(out.cpu(), 5.0 + G.colsum_ref(part.reshape(-1)[D:], nblk, D, 2 * D))
    assert torch.equal(out.cpu(), 5.0 + part[:, 1, :].sum(0))


@pytest.mark.parametrize("dtype", [BF, F32])
def test_colsum_real_values_against_float64(dtype):
    lib, check, ptr, stream, dt = _lib()
    rows, cols = G.COLSUM_REAL[dtype]
    g = torch.Generator().manual_seed(cols)
    x = (torch.randn(rows, cols, generator=g) * 3 + 0.5).to(dtype)
    x_d = x.cuda()
    (ref,), (err,) = R.e32(lambda a: G.colsum_ref(a, rows, cols, cols), (x.float(),))
    out = AR.guarded((cols,), F32, fill=0.0)
    _colsum(lib, check, stream, x_d.data_ptr(), rows, cols, cols, out, None, 1, dt(dtype))
    print(f"\ncolsum {dtype} {rows} x {cols}")
    _gate(f"colsum {dtype}", out, ref, err)


@pytest.mark.parametrize("rows", G.ROWSUM_ROWS)
def test_rowsum_f32_is_the_ordered_sum(rows):
    lib, check, ptr, stream, dt = _lib()
    g = torch.Generator().manual_seed(rows)
    for cols in G.ROWSUM_COLS:
        part = torch.randn(rows, cols, generator=g) * torch.logspace(-2, 2, cols)
        out0 = torch.randn(cols, generator=g)
        part_d = part.cuda()
        out = _guarded_copy(out0)
        check(lib.htrvt_rowsum_f32(ptr(part_d), rows, cols, ptr(out), stream()), "rowsum_f32")
        assert G.bits_mismatch(out.cpu().numpy(), G.rowsum_f32_ref(part.numpy(), out0.numpy())) == 0, cols


@pytest.mark.parametrize("dtype", [BF, F32])
def test_masked_rows_are_one_set_in_forward_backward_and_column_sum(dtype):
    """htrvt_mask_tokens_fwd, htrvt_mask_tokens_bwd and htrvt_colsum(keep, keep_mod = rows) on one per-sample mask holding 0,
    -0.0, 1 and 0.5: the rows replaced by the token, the rows zeroed and the rows summed are the same set"""
    lib, check, ptr, stream, dt = _lib()
    B, N, D = 3, 11, 40
    rows = B * N
    keep = torch.tensor([0.0, -0.0, 1.0, 0.5]).repeat(rows)[:rows].clone()
    masked = torch.tensor([k % 4 < 2 for k in range(rows)])
    g = torch.Generator().manual_seed(D)
    x = torch.randint(-3, 4, (rows, D), generator=g).to(dtype)
    token = torch.full((D,), 9.0)
    dy = torch.zeros(rows, D)
    dy[:, rows:] = torch.randint(-3, 4, (rows, D - rows), generator=g).float()
    dy[torch.arange(rows), torch.arange(rows)] = 2.0                      # column r of the sum names row r
    dy = dy.to(dtype)
    x_d, dy_d, keep_d, token_d = x.cuda(), dy.cuda(), keep.cuda(), token.cuda()
    y, dx = AR.guarded((rows, D), dtype), AR.guarded((rows, D), dtype)
    check(lib.htrvt_mask_tokens_fwd(ptr(x_d), ptr(keep_d), rows, ptr(token_d), ptr(y), rows, D, dt(dtype), stream()), "mask_tokens_fwd")
    check(lib.htrvt_mask_tokens_bwd(ptr(dy_d), ptr(keep_d), rows, ptr(dx), rows, D, dt(dtype), stream()), "mask_tokens_bwd")
    out = AR.guarded((D,), F32, fill=0.0)
    _colsum(lib, check, stream, dy_d.data_ptr(), rows, D, D, out, keep_d, rows, dt(dtype))
    replaced = (y.cpu().float() == 9).all(1)
    zeroed = (dx.cpu().float() == 0).all(1)
    summed = out.cpu()[:rows] == 2
    assert torch.equal(replaced, masked) and torch.equal(zeroed, masked) and torch.equal(summed, masked)
    assert torch.equal(out.cpu(), G.colsum_ref(dy.float(), rows, D, D, keep, rows))
    assert G.bits_mismatch(y, G.mask_tokens_fwd_ref(x, keep, rows, token)) == 0
    assert G.bits_mismatch(dx, G.mask_tokens_bwd_ref(dy, keep, rows)) == 0


# ==========================================================================================================================
# token masking
# ==========================================================================================================================
def _mask_case(lib, check, ptr, stream, dti, x, keep, keep_mod, token):
    rows, D = x.shape
    x_d, keep_d, token_d = x.cuda(), keep.cuda(), token.cuda()
    y, dx = AR.guarded((rows, D), x.dtype), AR.guarded((rows, D), x.dtype)
    check(lib.htrvt_mask_tokens_fwd(ptr(x_d), ptr(keep_d), keep_mod, ptr(token_d), ptr(y), rows, D, dti, stream()), "mask_tokens_fwd")
    check(lib.htrvt_mask_tokens_bwd(ptr(x_d), ptr(keep_d), keep_mod, ptr(dx), rows, D, dti, stream()), "mask_tokens_bwd")
    assert G.bits_mismatch(y, G.mask_tokens_fwd_ref(x, keep, keep_mod, token)) == 0
    want = G.mask_tokens_bwd_ref(x, keep, keep_mod)
    assert G.bits_mismatch(dx, want) == 0
    masked = keep[torch.arange(rows) % keep_mod] == 0
    assert _zero_bits(dx.cpu()[masked])


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("dtype,B,N,D", [(d, *c) for d in (BF, F32) for c in G.MASK_SMALL[d]])
def test_mask_tokens_small_shapes(dtype, B, N, D, per_sample, flip):
    """the source carries NaN, infinities and the rounding edges: kept rows pass through bit for bit, masked rows are the
    token (rounded once) or exactly +0, whatever the source row held"""
    lib, check, ptr, stream, dt = _lib()
    rows = B * N
    keep_mod = rows if per_sample else N
    keep = ((torch.arange(keep_mod) % 3 != 0) != flip).float()
    x = G.with_edges((rows, D), rows * D).to(dtype)
    token = G.with_edges((D,), D + 1)
    _mask_case(lib, check, ptr, stream, dt(dtype), x, keep, keep_mod, token)


def test_mask_tokens_past_the_block_cap():
    lib, check, ptr, stream, dt = _lib()
    rows, D = G.MASK_BIG
    assert rows * (D // 4) > G.MASK_BLOCK_CAP * 256
    keep = (torch.arange(rows) % 3 != 0).float()
    x = G.with_edges((rows, D), 77)
    _mask_case(lib, check, ptr, stream, dt(F32), x, keep, rows, torch.tensor([1.5, -2.25, 3.0, 1e-3]))


@pytest.mark.parametrize("dtype", [BF, F32])
def test_mask_tokens_without_rows_writes_nothing(dtype):
    lib, check, ptr, stream, dt = _lib()
    D = 8
    x, keep, token = torch.ones(4, D, dtype=dtype, device="cuda"), torch.zeros(4, device="cuda"), torch.ones(D, device="cuda")
    y = AR.guarded((4, D), dtype, fill=7.0)
    assert lib.htrvt_mask_tokens_fwd(ptr(x), ptr(keep), 4, ptr(token), ptr(y), 0, D, dt(dtype), stream()) == 0
    assert lib.htrvt_mask_tokens_bwd(ptr(x), ptr(keep), 4, ptr(y), 0, D, dt(dtype), stream()) == 0
    torch.cuda.synchronize()
    assert bool((y == 7).all())


# ==========================================================================================================================
# dense relative-position bias
# ==========================================================================================================================
@pytest.mark.parametrize("case", G.RELPOS_CASES)
def test_relpos_bias_forward_and_backward(case):
    lib, check, ptr, stream, dt = _lib()
    N, P, ws, shift, ld, heads = case
    table = (torch.arange((2 * P - 1) * heads, dtype=F32) + 1).view(2 * P - 1, heads)         # distinct: the output is a gather
    table_d = _guarded_copy(table)
    bias = AR.guarded((heads, ld, ld), F32)
    dtable = AR.guarded((2 * P - 1, heads), F32, fill=7.0)
    if not G.relpos_in_contract(case):
        # a window wider than num_patches: refused before any launch (checked on the CPU first), nothing written
        dbias_d = torch.zeros(heads, ld, ld, device="cuda")
        assert lib.htrvt_relpos_bias_fwd(ptr(table_d), ptr(bias), N, P, ws, shift, heads, ld, stream()) != 0
        assert "window" in lib.htrvt_last_error().decode()
        assert lib.htrvt_relpos_bias_bwd(ptr(dbias_d), ptr(dtable), N, P, ws, shift, heads, ld, stream()) != 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(bias).all()) and bool((dtable == 7).all())
        return
    check(lib.htrvt_relpos_bias_fwd(ptr(table_d), ptr(bias), N, P, ws, shift, heads, ld, stream()), "relpos_bias_fwd")
    assert torch.equal(bias.cpu(), G.relpos_bias_ref(table, N, P, ws, shift, ld))           # padding rows and columns included

    g = torch.Generator().manual_seed(N + P + ws)
    inside = G.relpos_attending(N, P, ws, shift)
    dbias = torch.full((heads, ld, ld), NAN)                        # NaN wherever no pair attends: none may reach the result
    dbias[:, :N, :N] = torch.where(inside[None], torch.randint(-3, 4, (heads, N, N), generator=g).float(), torch.tensor(NAN))
    dbias_d = dbias.cuda()
    want = G.relpos_bias_bwd_ref(dbias, N, P, ws, shift, ld)
    check(lib.htrvt_relpos_bias_bwd(ptr(dbias_d), ptr(dtable), N, P, ws, shift, heads, ld, stream()), "relpos_bias_bwd")
    assert torch.equal(dtable.cpu(), want)                          # all 2P-1 rows overwritten, unused entries 0
    again = AR.guarded((2 * P - 1, heads), F32, fill=-3.0)
    check(lib.htrvt_relpos_bias_bwd(ptr(dbias_d), ptr(again), N, P, ws, shift, heads, ld, stream()), "relpos_bias_bwd")
    assert G.bits_mismatch(again, dtable) == 0


# ==========================================================================================================================
# optimizer and SAM
# ==========================================================================================================================
def _scalars(lib, lr, b1, b2, eps, wd, step):
    out = (ctypes.c_float * 8)()
    assert lib.htrvt_adamw_scalars(lr, b1, b2, eps, wd, step, ctypes.addressof(out)) == 0
    return torch.from_numpy(np.frombuffer(out, dtype=np.float32).copy())


@pytest.mark.parametrize("wd", G.ADAMW_WD)
@pytest.mark.parametrize("n", G.ADAMW_N)
def test_adamw_and_adamw_dev_bit_for_bit(n, wd):
    """three steps, p / m / v after every step against glue_refs.adamw_ref (numpy float32, one rounding per operation),
    htrvt_adamw_dev on a device copy of htrvt_adamw_scalars' output against both; then the device scalars are changed
    between two htrvt_adamw_dev launches (what a replayed graph relies on)"""
    lib, check, ptr, stream, dt = _lib()
    H = G.ADAMW_HYPER
    p0, grads = G.adamw_inputs(n, n % 1000 + int(wd * 10))
    zeros = np.zeros(n, np.float32)
    ref = (p0.copy(), zeros.copy(), zeros.copy())
    host = [_guarded_copy(torch.from_numpy(a)) for a in ref]
    dev = [_guarded_copy(torch.from_numpy(a)) for a in ref]
    hyper = torch.zeros(8, device="cuda")
    for step, g in enumerate(grads, 1):
        g_d = torch.from_numpy(g).cuda()
        ref = G.adamw_ref(ref[0], g, ref[1], ref[2], H["lr"], H["b1"], H["b2"], H["eps"], wd, step)
        if step == 1:
            assert g[0] == 0 and ref[2][0] == 0          # a zero first gradient: v = 0, so denom = eps there
        check(lib.htrvt_adamw(ptr(host[0]), ptr(g_d), ptr(host[1]), ptr(host[2]), n, H["lr"], H["b1"], H["b2"], H["eps"], wd, step,
                              stream()), "adamw")
        hyper.copy_(_scalars(lib, H["lr"], H["b1"], H["b2"], H["eps"], wd, step))
        check(lib.htrvt_adamw_dev(ptr(dev[0]), ptr(g_d), ptr(dev[1]), ptr(dev[2]), n, ptr(hyper), stream()), "adamw_dev")
        for name, h, d, r in zip("pmv", host, dev, ref):
            bad = G.bits_mismatch(h.cpu().numpy(), r)
            assert bad == 0, f"htrvt_adamw step {step}: {bad} of {n} elements of {name} differ from the float32 restatement"
            assert G.bits_mismatch(d, h) == 0, f"htrvt_adamw_dev step {step}: {name} differs from htrvt_adamw"
    # new scalars in the same device buffer: the next launch must use them
    lr2, step2 = 3e-4, 7
    hyper.copy_(_scalars(lib, lr2, H["b1"], H["b2"], H["eps"], wd, step2))
    g_d = torch.from_numpy(grads[0]).cuda()
    check(lib.htrvt_adamw_dev(ptr(dev[0]), ptr(g_d), ptr(dev[1]), ptr(dev[2]), n, ptr(hyper), stream()), "adamw_dev")
    want = G.adamw_ref(ref[0], grads[0], ref[1], ref[2], lr2, H["b1"], H["b2"], H["eps"], wd, step2)
    stale = G.adamw_ref(ref[0], grads[0], ref[1], ref[2], H["lr"], H["b1"], H["b2"], H["eps"], wd, 3)
    assert G.bits_mismatch(stale[0], want[0]) > 0
    for name, d, r in zip("pmv", dev, want):
        assert G.bits_mismatch(d.cpu().numpy(), r) == 0, f"htrvt_adamw_dev after new scalars: {name}"


@pytest.mark.parametrize("n", G.SAM_N)
def test_sumsq_sam_first_step_and_restore(n):
    lib, check, ptr, stream, dt = _lib()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen) * 0.05
    g = torch.randn(n, generator=gen) * 3e-3
    g_d = g.cuda()
    nblk = lib.htrvt_sumsq_blocks(n)
    assert nblk == min(max((n // 4 + 255) // 256, 1), 1024)
    partial_ = AR.guarded((nblk,), F32)
    nsq, nsq2 = AR.guarded((1,), F32), AR.guarded((1,), F32)
    check(lib.htrvt_sumsq(ptr(g_d), n, ptr(partial_), ptr(nsq), stream()), "sumsq")
    check(lib.htrvt_sumsq(ptr(g_d), n, ptr(partial_), ptr(nsq2), stream()), "sumsq")
    want = float((g.double() ** 2).sum())
    assert abs(float(nsq) - want) <= 4 * EPS32 * want, (float(nsq), want)
    assert G.bits_mismatch(nsq, nsq2) == 0
    for rho in (0.05, 0.0):
        p, old = _guarded_copy(p0), AR.guarded((n,), F32)
        check(lib.htrvt_sam_first_step(ptr(p), ptr(g_d), ptr(old), n, rho, ptr(nsq), stream()), "sam_first_step")
        assert G.bits_mismatch(old, p0) == 0
        assert G.bits_mismatch(p.cpu().numpy(), G.sam_climb_ref(p0.numpy(), g.numpy(), float(nsq), rho)) == 0
        if rho == 0.0:
            assert G.bits_mismatch(p, p0) == 0
        check(lib.htrvt_sam_restore(ptr(p), ptr(old), n, stream()), "sam_restore")
        assert G.bits_mismatch(p, p0) == 0


# ==========================================================================================================================
# float32 element-wise steps
# ==========================================================================================================================
@pytest.mark.parametrize("n", G.ELEMENTWISE_N)
def test_elementwise_f32_per_element(n):
    lib, check, ptr, stream, dt = _lib()
    # With four elements E32 is the float32 error of ONE of them and can be any number down to 0: the inputs are redrawn while
    # a draw is below 2^-26 (a gate under the spacing of the float32 the kernel stores) -- tests/test_dropnorm_gpu.py's rule
    # for its one-row statistics; it reads the reference alone.
    for seed in range(n, n + 64000, 1000):
        a, b = G.elementwise_inputs(n, seed)
        if min(R.e32(G.gelu_ref, (a,))[1][0], R.e32(G.gelu_grad_mul_ref, (a, b))[1][0]) >= 2.0 ** -26:
            break
    else:
        raise AssertionError("no draw with E32 >= 2^-26")
    a_d, b_d = a.cuda(), b.cuda()
    print(f"\nelementwise_f32 n={n} (seed {seed})")
    out = AR.guarded((n,), F32)
    check(lib.htrvt_elementwise_f32(ptr(a_d), None, ptr(out), n, 0, stream()), "gelu")
    (ref,), (err,) = R.e32(G.gelu_ref, (a,))
    _gate("gelu", out, ref, err)
    out = AR.guarded((n,), F32)
    check(lib.htrvt_elementwise_f32(ptr(a_d), ptr(b_d), ptr(out), n, 1, stream()), "gelu'")
    (ref,), (err,) = R.e32(G.gelu_grad_mul_ref, (a, b))
    _gate("a * gelu'(b)", out, ref, err)
    out = AR.guarded((n,), F32)
    check(lib.htrvt_elementwise_f32(ptr(a_d), ptr(b_d), ptr(out), n, 2, stream()), "add")
    assert G.bits_mismatch(out, a + b) == 0
    check(lib.htrvt_elementwise_f32(ptr(out), ptr(b_d), ptr(out), n, 2, stream()), "add in place")
    assert G.bits_mismatch(out, (a + b) + b) == 0
