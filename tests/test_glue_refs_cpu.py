"""tests/glue_refs.py without a GPU: every reference against torch's own operators or float64 autograd, the comparisons of
tests/test_glue_kernels_gpu.py against a list of injected faults (each must be rejected), htrvt_adamw_scalars (host only) bit
for bit, and the argument checks of every glue entry point: a bad call returns non-zero with the reason in
htrvt_last_error() BEFORE any launch -- which is why these calls can be made here, with host addresses that are never read.
The GPU file never passes such arguments."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_refs as G

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS32 = 2.0 ** -24
IN_CONTRACT = [c for c in G.RELPOS_CASES if G.relpos_in_contract(c)]
REFUSED = [c for c in G.RELPOS_CASES if not G.relpos_in_contract(c)]


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import _lib
    return _lib.lib


def _variants():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import variants
    return variants


# ---- the references ------------------------------------------------------------------------------------------------------
def test_edge_values_hold_the_named_patterns_and_torch_rounds_them_to_nearest_even():
    e = G.bf16_edge_values()
    bits = set(int(b) for b in e.numpy().view(np.uint32))
    for b in (0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF,
              0x7F800000):
        assert b in bits and (b | 0x80000000) in bits, hex(b)
    assert 0x7FC00000 in bits

    def rounded(b):
        x = torch.from_numpy(np.array([b], dtype=np.uint32).view(np.float32).copy())
        return int(x.to(BF).view(torch.int16).numpy().view(np.uint16)[0])
    assert rounded(0x3F808000) == 0x3F80 and rounded(0x3F818000) == 0x3F82 and rounded(0x3FFF8000) == 0x4000
    assert rounded(0x3F807FFF) == 0x3F80 and rounded(0x3F808001) == 0x3F81
    assert rounded(0x7F7FFFFF) == 0x7F80 and rounded(0xFF7FFFFF) == 0xFF80 and rounded(0x7F7F7FFF) == 0x7F7F
    assert rounded(0x80000000) == 0x8000 and rounded(0x00008000) == 0x0000 and rounded(0x00018000) == 0x0002
    assert rounded(0x007FFFFF) == 0x0080
    assert torch.isnan(e.to(BF)[-1])
    x = G.with_edges((37, 24), 1)
    assert G.bf16_mismatch(x.to(BF), x) == 0
    assert torch.isnan(x).sum() >= 4 and torch.isinf(x).sum() >= 8


def test_split_reference_recovers_x_to_two_to_the_minus_sixteen():
    x = G.with_edges((64, 40), 2)
    hi, lo = G.split_bf16_ref(x)
    normal = torch.isfinite(x) & (x.abs() >= 2.0 ** -126) & torch.isfinite(hi.float())
    d = (hi.double() + lo.double() - x.double()).abs()
    assert bool((d[normal] <= 2.0 ** -16 * x.double().abs()[normal]).all())
    big = torch.isinf(hi.float())
    assert bool((lo.float()[big] == 0).all()) and bool(torch.isinf(hi.float() + lo.float())[big].all())


@pytest.mark.parametrize("dtype", [F32, F64])
def test_colsum_ref_is_the_sum_of_the_selected_rows(dtype):
    g = torch.Generator().manual_seed(3)
    rows, cols, ld = 257, 24, 40
    x = torch.randn(rows, ld, generator=g).to(dtype)
    assert torch.equal(G.colsum_ref(x, rows, cols, ld), x[:, :cols].sum(0))
    for keep_mod in (16, rows):
        keep = (torch.rand(keep_mod, generator=g) > 0.4).float()
        sel = torch.tensor([float(keep[r % keep_mod]) == 0.0 for r in range(rows)])
        want = x[sel][:, :cols].sum(0)
        got = G.colsum_ref(x, rows, cols, ld, keep, keep_mod)
        assert got.dtype == dtype and torch.equal(got, want)
    # the flat form behind an offset: the second half of every [2 D] row
    D, nblk = 12, 9
    part = torch.randn(nblk, 2, D, generator=g).to(dtype)
    assert torch.equal(G.colsum_ref(part.reshape(-1)[D:], nblk, D, 2 * D), part[:, 1, :].sum(0))
    assert [G.colsum_splits(r) for r in (1, 255, 256, 257, 8191, 8192, 8193, 12345)] == [1, 1, 2, 2, 63, 64, 64, 64]


def test_colsum_case_selection_rule():
    for dtype in (BF, F32):
        cases = G.colsum_cases(dtype)
        for rows in G.COLSUM_ROWS:
            assert len({c for r, c, _ in cases if r == rows}) == 2
        for cols in G.COLSUM_COLS[dtype]:
            assert len({r for r, c, _ in cases if c == cols}) >= 3
            assert {ld - c for r, c, ld in cases if c == cols} == {0, 16}


def test_rowsum_ref_is_an_ordered_float32_sum():
    g = torch.Generator().manual_seed(4)
    part = torch.randn(17, 65, generator=g).numpy()
    out = torch.randn(65, generator=g).numpy()
    got = G.rowsum_f32_ref(part, out)
    assert got.dtype == np.float32
    acc = np.float32(0)
    for r in range(17):
        acc = np.float32(acc + part[r, 5])
    assert got[5] == np.float32(out[5] + acc)
    assert np.abs(got.astype(np.float64) - (part.astype(np.float64).sum(0) + out)).max() <= 18 * EPS32 * np.abs(part).sum(0).max()


@pytest.mark.parametrize("case", IN_CONTRACT)
def test_relpos_reference_agrees_with_the_index_bookkeeping(case):
    """two independent statements: windows built by pad / roll / view, and the modulus formula of variants.py"""
    N, P, ws, shift, ld, heads = case
    V = _variants()
    idx, inside = V.relative_position_index(N, P, ws, shift)
    table = (torch.arange((2 * P - 1) * heads, dtype=F32) + 1).view(2 * P - 1, heads)
    bias = G.relpos_bias_ref(table, N, P, ws, shift, ld)
    assert bias.shape == (heads, ld, ld)
    want = torch.where(inside[None], table[idx.clamp(0, 2 * P - 2)].permute(2, 0, 1), torch.tensor(G.MASKED))
    assert bool(((idx >= 0) & (idx <= 2 * P - 2))[inside].all())
    assert torch.equal(bias[:, :N, :N], want)
    assert torch.equal(G.relpos_attending(N, P, ws, shift), inside)
    assert bool((bias[:, :, N:] == G.MASKED).all())
    assert bool((bias[:, N:, 0] == 0).all()) and bool((bias[:, N:, 1:] == G.MASKED).all())


@pytest.mark.parametrize("case", REFUSED)
def test_a_window_wider_than_the_table_is_outside_both_statements(case):
    """the reference model raises for it (a window of ws > num_patches tokens), the restatement raises, and the modulus
    formula names entries outside the 2 P - 1 rows of the table for attending pairs: nothing defines a result"""
    N, P, ws, shift, ld, heads = case
    with pytest.raises(ValueError):
        G.window_layout(N, P, ws, shift)
    idx, inside = _variants().relative_position_index(N, P, ws, shift)
    assert bool(((idx < 0) | (idx > 2 * P - 2))[inside].any())


@pytest.mark.parametrize("case", IN_CONTRACT)
def test_relpos_backward_reference_is_the_autograd_of_the_forward(case):
    N, P, ws, shift, ld, heads = case
    g = torch.Generator().manual_seed(N + P + ws)
    inside = G.relpos_attending(N, P, ws, shift)
    dbias = torch.full((heads, ld, ld), float("nan"), dtype=F64)
    dbias[:, :N, :N] = torch.where(inside[None], torch.randn(heads, N, N, generator=g, dtype=F64), torch.tensor(float("nan"), dtype=F64))
    table = torch.randn(2 * P - 1, heads, generator=g, dtype=F64).requires_grad_(True)
    bias = G.relpos_bias_ref(table, N, P, ws, shift, ld)
    zero = torch.zeros((), dtype=F64)
    (torch.where(inside[None], bias[:, :N, :N], zero) * torch.where(inside[None], dbias[:, :N, :N], zero)).sum().backward()
    got = G.relpos_bias_bwd_ref(dbias, N, P, ws, shift, ld)
    assert not torch.isnan(got).any()
    assert torch.allclose(got, table.grad, rtol=1e-12, atol=1e-12)


def test_adamw_reference_within_eight_ulp_of_torch_optim():
    """the rule of test_adamw_kernel_matches_torch_optim: ATen's CPU kernels contract to FMA, so not bit for bit.  Every step
    starts from torch's own state: m + w (g - m) cancels where g ~ -9 m, and a last-bit difference of an earlier step would
    then be many ulps of the small m a later step starts from -- a difference of the trajectories, not of the step."""
    n = 4096
    p0, grads = G.adamw_inputs(n, 11)
    p_ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([p_ref], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.5, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step, g in enumerate(grads, 1):
        if step > 1:
            p, m, v = (t.detach().numpy().copy() for t in (p_ref, opt.state[p_ref]["exp_avg"], opt.state[p_ref]["exp_avg_sq"]))
        m_prev, v_prev = torch.from_numpy(m.copy()), torch.from_numpy(v.copy())
        p_ref.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = G.adamw_ref(p, g, m, v, 1e-3, 0.9, 0.99, 1e-8, 0.5, step)
        st = opt.state[p_ref]
        gt = torch.from_numpy(g)
        scales = {"p": torch.maximum(p_ref.detach().abs(), torch.full((n,), 1e-3)),
                  "m": torch.maximum(torch.maximum(st["exp_avg"].abs(), m_prev.abs()), gt.abs()),
                  "v": torch.maximum(torch.maximum(st["exp_avg_sq"], v_prev), gt * gt)}
        for name, got, ref in (("p", p, p_ref.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            d = (torch.from_numpy(got) - ref).abs()
            assert bool((d <= 8 * EPS32 * scales[name] + 1e-37).all()), (step, name, float(d.max()))


def test_gelu_references_against_torch():
    x = torch.linspace(-9, 9, 4001, dtype=F64)
    assert torch.allclose(G.gelu_ref(x), F.gelu(x), rtol=1e-13, atol=1e-15)
    b = x.clone().requires_grad_(True)
    F.gelu(b).sum().backward()
    a = torch.linspace(2, -3, 4001, dtype=F64)
    assert torch.allclose(G.gelu_grad_mul_ref(a, x), a * b.grad, rtol=1e-12, atol=1e-15)
    a32, b32 = G.elementwise_inputs(1028, 1)
    assert a32.dtype == F32 and float(a32.min()) < -8 and float(a32.max()) > 8 and float(b32.max()) > 8


def test_sam_reference_is_reciprocal_then_multiply():
    nsq, rho = np.float32(3.7e-4), 0.05
    s = G.sam_scale_ref(nsq, rho)
    assert s.dtype == np.float32
    t = torch.tensor(float(nsq), dtype=F32)
    assert float(s) == float(rho / (t.sqrt() + 1e-12))      # torch's float / tensor on the host
    p, g = np.float32([1.0, -2.0]), np.float32([0.5, 0.25])
    assert np.array_equal(G.sam_climb_ref(p, g, nsq, rho), p + (g * s).astype(np.float32))
    assert np.array_equal(G.sam_climb_ref(p, g, nsq, 0.0), p)


def test_case_lists_contain_the_named_edges():
    assert G.CAST_N[-1] > G.CAST_BLOCK_CAP * G.CAST_THREADS and {1, 255, 257} <= set(G.CAST_N)
    assert (60, 70, 72) in G.CAST_TRANSPOSE_CASES and (1, 1, 8) in G.CAST_TRANSPOSE_CASES
    assert {127, 128, 255, 256, 257, 8191, 8192, 8193} <= set(G.COLSUM_ROWS)
    assert G.MASK_BIG[0] * (G.MASK_BIG[1] // 4) > G.MASK_BLOCK_CAP * 256
    assert G.ADAMW_N[-1] // 4 > 2048 * 256 and G.SAM_N[-1] // 4 > 2048 * 256
    assert all(n % 4 == 0 for n in G.ADAMW_N + G.SAM_N + G.ELEMENTWISE_N)
    assert (20, 20, 32, 5, 24, 2) in G.RELPOS_CASES and len(G.RELPOS_CASES) == 9 and len(REFUSED) == 1


# ---- injected faults: the comparisons of the GPU file must reject each ----------------------------------------------------
def test_fault_bf16_truncation_instead_of_rne():
    x = G.with_edges((33, 24), 5)
    trunc = (x.view(torch.int32) >> 16).to(torch.int16).view(BF)
    bad = G.bf16_mismatch(trunc, x)
    print(f"truncation: {bad} of {x.numel()} elements differ")
    assert bad > x.numel() // 4
    # and on the integers in [-64, 64) of the older tests it is invisible
    ints = torch.randint(-64, 64, (33, 24)).float()
    assert G.bf16_mismatch((ints.view(torch.int32) >> 16).to(torch.int16).view(BF), ints) == 0


def test_fault_nan_flushed_to_zero():
    x = G.with_edges((33, 24), 6)
    got = torch.nan_to_num(x, nan=0.0, posinf=float("inf"), neginf=float("-inf")).to(BF)
    assert G.bf16_mismatch(got, x) == int(torch.isnan(x).sum()) > 0
    assert G.bits_mismatch(torch.nan_to_num(x, nan=0.0, posinf=float("inf"), neginf=float("-inf")), x) == int(torch.isnan(x).sum())


def test_fault_colsum_drops_the_last_row_of_the_last_split():
    g = torch.Generator().manual_seed(7)
    rows, cols = 8193, 24
    x = torch.randint(-3, 4, (rows, cols), generator=g).float()
    x[-1, 3] = 2.0
    assert not torch.equal(G.colsum_ref(x, rows - 1, cols, cols), G.colsum_ref(x, rows, cols, cols))


def test_fault_colsum_sums_the_kept_rows():
    g = torch.Generator().manual_seed(8)
    rows, cols = 257, 24
    x = torch.randint(-3, 4, (rows, cols), generator=g).float()
    keep = (torch.arange(16) % 3 != 0).float()
    assert not torch.equal(G.colsum_ref(x, rows, cols, cols, 1.0 - keep, 16), G.colsum_ref(x, rows, cols, cols, keep, 16))


def test_fault_relpos_shift_of_the_wrong_sign():
    seen = 0
    for case in IN_CONTRACT:
        N, P, ws, shift, ld, heads = case
        if shift == 0 or 2 * shift == ws:       # half a window either way is the same partition
            continue
        seen += 1
        table = (torch.arange((2 * P - 1) * heads, dtype=F32) + 1).view(2 * P - 1, heads)
        assert not torch.equal(G.relpos_bias_ref(table, N, P, ws, shift, ld, _roll_sign=+1), G.relpos_bias_ref(table, N, P, ws, shift, ld)), case
    assert seen >= 2


def test_fault_relpos_backward_accumulates_into_its_destination():
    N, P, ws, shift, ld, heads = 100, 128, 12, 11, 128, 2
    inside = G.relpos_attending(N, P, ws, shift)
    dbias = torch.full((heads, ld, ld), float("nan"))
    dbias[:, :N, :N] = torch.where(inside[None], torch.randint(-3, 4, (heads, N, N)).float(), torch.tensor(float("nan")))
    want = G.relpos_bias_bwd_ref(dbias, N, P, ws, shift, ld)
    assert bool((want[:P - ws] == 0).all())                 # entries no pair uses: the pre-fill would show there
    assert not torch.equal(want + 7.0, want)


def test_fault_adamw_with_an_fma_in_the_v_update():
    n = 1020
    p0, grads = G.adamw_inputs(n, 3)
    z = np.zeros(n, np.float32)
    p1, m1, v1 = G.adamw_ref(p0, grads[0], z, z, 1e-3, 0.9, 0.99, 1e-8, 0.5, 1)      # v = 0 hides an FMA: take the second step
    g2 = grads[1]
    want = G.adamw_ref(p1, g2, m1, v1, 1e-3, 0.9, 0.99, 1e-8, 0.5, 2)
    got = G.adamw_ref(p1, g2, m1, v1, 1e-3, 0.9, 0.99, 1e-8, 0.5, 2, _fma_v=True)
    assert G.bits_mismatch(got[2], want[2]) > 0
    print(f"FMA in v: {G.bits_mismatch(got[2], want[2])} of {n} elements of v, {G.bits_mismatch(got[0], want[0])} of p differ")


# ---- htrvt_adamw_scalars: host only -------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.5, 0.0])
@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
def test_adamw_scalars_bit_for_bit(step, wd):
    lib = _lib()
    out = (ctypes.c_float * 8)(*([7.0] * 8))
    assert lib.htrvt_adamw_scalars(1e-3, 0.9, 0.99, 1e-8, wd, step, ctypes.addressof(out)) == 0
    got = np.frombuffer(out, dtype=np.float32)
    want = G.adamw_scalars_ref(1e-3, 0.9, 0.99, 1e-8, wd, step)
    assert want.shape == (8,) and want[7] == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


# ---- refusals ------------------------------------------------------------------------------------------------------------
_HOST = ctypes.create_string_buffer(1 << 12)
A = (ctypes.addressof(_HOST) + 63) // 64 * 64      # a non-null, 64-byte aligned address; a refused call never reads it


def _refused(lib, name, call):
    """non-zero, and htrvt_last_error() set by THIS call to a reason of the entry point's own (not a failed launch)"""
    out = (ctypes.c_float * 8)()
    assert lib.htrvt_adamw_scalars(1e-3, 0.9, 0.99, 1e-8, 0.5, 0, ctypes.addressof(out)) != 0      # a known message first
    sentinel = lib.htrvt_last_error().decode()
    assert "htrvt_adamw_scalars" in sentinel
    rc = call()
    err = lib.htrvt_last_error().decode()
    assert rc != 0, f"{name}: accepted"
    assert err and err != sentinel and "launch failed" not in err, (name, err)


def test_adamw_scalars_refuses_step_zero_and_a_null_output():
    lib = _lib()
    out = (ctypes.c_float * 8)()
    assert lib.htrvt_adamw_scalars(1e-3, 0.9, 0.99, 1e-8, 0.5, 0, ctypes.addressof(out)) != 0
    assert "htrvt_adamw_scalars" in lib.htrvt_last_error().decode()
    _refused(lib, "adamw (marker)", lambda: lib.htrvt_adamw(A, A, A, A, 6, 1e-3, 0.9, 0.99, 1e-8, 0.5, 1, None))
    assert lib.htrvt_adamw_scalars(1e-3, 0.9, 0.99, 1e-8, 0.5, 1, None) != 0
    assert "htrvt_adamw_scalars" in lib.htrvt_last_error().decode()


def _bad_calls(lib):
    BFt, F = 1, 0
    c = {}
    # htrvt_colsum(x, rows, cols, ld, out, keep, keep_mod, dtype, workspace, stream)
    c["colsum null x"] = lambda: lib.htrvt_colsum(None, 8, 8, 8, A, None, 1, BFt, None, None)
    c["colsum null out"] = lambda: lib.htrvt_colsum(A, 8, 8, 8, None, None, 1, BFt, None, None)
    c["colsum bf16 cols off the vector"] = lambda: lib.htrvt_colsum(A, 8, 12, 16, A, None, 1, BFt, None, None)
    c["colsum f32 cols off the vector"] = lambda: lib.htrvt_colsum(A, 8, 6, 8, A, None, 1, F, None, None)
    c["colsum ld off the vector"] = lambda: lib.htrvt_colsum(A, 8, 8, 12, A, None, 1, BFt, None, None)
    c["colsum ld < cols"] = lambda: lib.htrvt_colsum(A, 8, 16, 8, A, None, 1, BFt, None, None)
    c["colsum negative rows"] = lambda: lib.htrvt_colsum(A, -1, 8, 8, A, None, 1, BFt, None, None)
    c["colsum 256 rows without a workspace"] = lambda: lib.htrvt_colsum(A, 256, 8, 8, A, None, 1, BFt, None, None)
    c["colsum dtype"] = lambda: lib.htrvt_colsum(A, 8, 8, 8, A, None, 1, 2, None, None)
    c["colsum keep_mod 0 with a filter"] = lambda: lib.htrvt_colsum(A, 8, 8, 8, A, A, 0, BFt, None, None)
    c["rowsum null partial"] = lambda: lib.htrvt_rowsum_f32(None, 4, 8, A, None)
    c["rowsum null out"] = lambda: lib.htrvt_rowsum_f32(A, 4, 8, None, None)
    c["rowsum no columns"] = lambda: lib.htrvt_rowsum_f32(A, 4, 0, A, None)
    c["rowsum negative rows"] = lambda: lib.htrvt_rowsum_f32(A, -1, 8, A, None)
    c["cast_f32 null src"] = lambda: lib.htrvt_cast_f32(None, A, 8, BFt, None)
    c["cast_f32 null dst"] = lambda: lib.htrvt_cast_f32(A, None, 8, BFt, None)
    c["cast_f32 to float32"] = lambda: lib.htrvt_cast_f32(A, A, 8, F, None)
    c["cast_f32 dtype"] = lambda: lib.htrvt_cast_f32(A, A, 8, 2, None)
    c["cast_f32 negative n"] = lambda: lib.htrvt_cast_f32(A, A, -4, BFt, None)
    # htrvt_mask_tokens_fwd(x, keep, keep_mod, token, y, rows, D, dtype, stream) / _bwd(dy, keep, keep_mod, dx, rows, D, dtype, stream)
    for name, fn in (("fwd", lambda x, k, km, y, rows, D, dt: lib.htrvt_mask_tokens_fwd(x, k, km, A, y, rows, D, dt, None)),
                     ("bwd", lambda x, k, km, y, rows, D, dt: lib.htrvt_mask_tokens_bwd(x, k, km, y, rows, D, dt, None))):
        c[f"mask_tokens_{name} null x"] = lambda fn=fn: fn(None, A, 4, A, 8, 8, BFt)
        c[f"mask_tokens_{name} null keep"] = lambda fn=fn: fn(A, None, 4, A, 8, 8, BFt)
        c[f"mask_tokens_{name} null y"] = lambda fn=fn: fn(A, A, 4, None, 8, 8, BFt)
        c[f"mask_tokens_{name} bf16 D off the vector"] = lambda fn=fn: fn(A, A, 4, A, 8, 12, BFt)
        c[f"mask_tokens_{name} f32 D off the vector"] = lambda fn=fn: fn(A, A, 4, A, 8, 6, F)
        c[f"mask_tokens_{name} keep_mod does not divide"] = lambda fn=fn: fn(A, A, 4, A, 10, 8, BFt)
        c[f"mask_tokens_{name} keep_mod above the rows"] = lambda fn=fn: fn(A, A, 16, A, 8, 8, BFt)
        c[f"mask_tokens_{name} keep_mod 0"] = lambda fn=fn: fn(A, A, 0, A, 8, 8, BFt)
        c[f"mask_tokens_{name} dtype"] = lambda fn=fn: fn(A, A, 4, A, 8, 8, 2)
        c[f"mask_tokens_{name} negative rows"] = lambda fn=fn: fn(A, A, 4, A, -8, 8, BFt)
    c["mask_tokens_fwd null token"] = lambda: lib.htrvt_mask_tokens_fwd(A, A, 4, None, A, 8, 8, BFt, None)
    # htrvt_relpos_bias_*(table / dbias, bias / dtable, N, P, window, shift, heads, ld, stream)
    for name, fn in (("fwd", lib.htrvt_relpos_bias_fwd), ("bwd", lib.htrvt_relpos_bias_bwd)):
        c[f"relpos_{name} null source"] = lambda fn=fn: fn(None, A, 32, 32, 0, 0, 1, 32, None)
        c[f"relpos_{name} null destination"] = lambda fn=fn: fn(A, None, 32, 32, 0, 0, 1, 32, None)
        c[f"relpos_{name} shift == window"] = lambda fn=fn: fn(A, A, 32, 32, 12, 12, 1, 32, None)
        c[f"relpos_{name} negative shift"] = lambda fn=fn: fn(A, A, 32, 32, 12, -1, 1, 32, None)
        c[f"relpos_{name} P < N"] = lambda fn=fn: fn(A, A, 32, 31, 0, 0, 1, 32, None)
        c[f"relpos_{name} ld < N"] = lambda fn=fn: fn(A, A, 32, 32, 0, 0, 1, 31, None)
        c[f"relpos_{name} no heads"] = lambda fn=fn: fn(A, A, 32, 32, 0, 0, 0, 32, None)
        for case in REFUSED:
            N, P, ws, shift, ld, heads = case
            c[f"relpos_{name} window wider than the table {case}"] = lambda fn=fn, a=(N, P, ws, shift, heads, ld): fn(A, A, *a, None)
    # htrvt_cast_transpose_f32(src, dst, dst_t, rows, cols, ld_t, dtype, stream)
    c["cast_transpose null src"] = lambda: lib.htrvt_cast_transpose_f32(None, A, A, 8, 8, 8, BFt, None)
    c["cast_transpose null dst_t"] = lambda: lib.htrvt_cast_transpose_f32(A, A, None, 8, 8, 8, BFt, None)
    c["cast_transpose ld_t < rows"] = lambda: lib.htrvt_cast_transpose_f32(A, A, A, 9, 8, 8, BFt, None)
    c["cast_transpose to float32"] = lambda: lib.htrvt_cast_transpose_f32(A, A, A, 8, 8, 8, F, None)
    c["cast_transpose no rows"] = lambda: lib.htrvt_cast_transpose_f32(A, A, A, 0, 8, 8, BFt, None)
    # htrvt_pack_conv_weight(w, fwd, dgrad, Co, Ci, taps, cpad_in, cpad_out, dtype, stream); _slots: ..., row_taps, tap0, dtype, stream
    c["pack null w"] = lambda: lib.htrvt_pack_conv_weight(None, A, A, 8, 8, 9, 8, 8, BFt, None)
    c["pack no output"] = lambda: lib.htrvt_pack_conv_weight(A, None, None, 8, 8, 9, 8, 8, BFt, None)
    c["pack cpad_in < Ci"] = lambda: lib.htrvt_pack_conv_weight(A, A, A, 8, 9, 9, 8, 8, BFt, None)
    c["pack cpad_out < Co"] = lambda: lib.htrvt_pack_conv_weight(A, A, A, 9, 8, 9, 8, 8, BFt, None)
    c["pack no taps"] = lambda: lib.htrvt_pack_conv_weight(A, A, A, 8, 8, 0, 8, 8, BFt, None)
    c["pack ten taps"] = lambda: lib.htrvt_pack_conv_weight(A, A, A, 8, 8, 10, 8, 8, BFt, None)
    c["pack dtype"] = lambda: lib.htrvt_pack_conv_weight(A, A, A, 8, 8, 9, 8, 8, 2, None)
    c["pack_slots tap0 + taps > row_taps"] = lambda: lib.htrvt_pack_conv_weight_slots(A, A, A, 8, 8, 9, 8, 8, 10, 2, BFt, None)
    c["pack_slots negative tap0"] = lambda: lib.htrvt_pack_conv_weight_slots(A, A, A, 8, 8, 9, 8, 8, 10, -1, BFt, None)
    c["pack_slots dtype"] = lambda: lib.htrvt_pack_conv_weight_slots(A, A, A, 8, 8, 9, 8, 8, 10, 1, 3, None)
    # htrvt_split_bf16(src, rows, cols, ld_src, cat, order, cat_f32, transpose, hi, lo, stream)
    c["split null src"] = lambda: lib.htrvt_split_bf16(None, 4, 8, 8, A, 0, 0, 0, None, None, None)
    c["split no output"] = lambda: lib.htrvt_split_bf16(A, 4, 8, 8, None, 0, 0, 0, None, None, None)
    c["split order 2"] = lambda: lib.htrvt_split_bf16(A, 4, 8, 8, A, 2, 0, 0, None, None, None)
    c["split ld_src < cols"] = lambda: lib.htrvt_split_bf16(A, 4, 8, 4, A, 0, 0, 0, None, None, None)
    c["split planes with a transpose"] = lambda: lib.htrvt_split_bf16(A, 4, 8, 8, A, 0, 0, 1, A, A, None)
    c["split planes off the vector"] = lambda: lib.htrvt_split_bf16(A, 4, 9, 9, None, 0, 0, 0, A, A, None)
    # htrvt_elementwise_f32(a, b, out, n, mode, stream)
    c["elementwise null a"] = lambda: lib.htrvt_elementwise_f32(None, A, A, 8, 2, None)
    c["elementwise null out"] = lambda: lib.htrvt_elementwise_f32(A, A, None, 8, 2, None)
    c["elementwise null b in mode 1"] = lambda: lib.htrvt_elementwise_f32(A, None, A, 8, 1, None)
    c["elementwise n % 4"] = lambda: lib.htrvt_elementwise_f32(A, A, A, 6, 2, None)
    c["elementwise n 0"] = lambda: lib.htrvt_elementwise_f32(A, A, A, 0, 2, None)
    c["elementwise mode 3"] = lambda: lib.htrvt_elementwise_f32(A, A, A, 8, 3, None)
    # htrvt_adamw(p, g, m, v, n, lr, b1, b2, eps, wd, step, stream); _dev(p, g, m, v, n, hyper, stream)
    H = (1e-3, 0.9, 0.99, 1e-8, 0.5)
    c["adamw n % 4"] = lambda: lib.htrvt_adamw(A, A, A, A, 6, *H, 1, None)
    c["adamw step 0"] = lambda: lib.htrvt_adamw(A, A, A, A, 8, *H, 0, None)
    for i, nm in enumerate("pgmv"):
        args = [A, A, A, A]
        args[i] = None
        c[f"adamw null {nm}"] = lambda args=tuple(args): lib.htrvt_adamw(*args, 8, *H, 1, None)
        c[f"adamw_dev null {nm}"] = lambda args=tuple(args): lib.htrvt_adamw_dev(*args, 8, A, None)
    c["adamw_dev n % 4"] = lambda: lib.htrvt_adamw_dev(A, A, A, A, 6, A, None)
    c["adamw_dev null scalars"] = lambda: lib.htrvt_adamw_dev(A, A, A, A, 8, None, None)
    # htrvt_sumsq(x, n, partial, out, stream); htrvt_sam_first_step(p, g, old, n, rho, norm_sq, stream); htrvt_sam_restore(p, old, n, stream)
    c["sumsq n % 4"] = lambda: lib.htrvt_sumsq(A, 6, A, A, None)
    c["sumsq n 0"] = lambda: lib.htrvt_sumsq(A, 0, A, A, None)
    c["sumsq null x"] = lambda: lib.htrvt_sumsq(None, 8, A, A, None)
    c["sumsq null partial"] = lambda: lib.htrvt_sumsq(A, 8, None, A, None)
    c["sumsq null out"] = lambda: lib.htrvt_sumsq(A, 8, A, None, None)
    c["sam_first_step n % 4"] = lambda: lib.htrvt_sam_first_step(A, A, A, 6, 0.05, A, None)
    c["sam_first_step negative rho"] = lambda: lib.htrvt_sam_first_step(A, A, A, 8, -0.05, A, None)
    c["sam_first_step null p"] = lambda: lib.htrvt_sam_first_step(None, A, A, 8, 0.05, A, None)
    c["sam_first_step null g"] = lambda: lib.htrvt_sam_first_step(A, None, A, 8, 0.05, A, None)
    c["sam_first_step null old"] = lambda: lib.htrvt_sam_first_step(A, A, None, 8, 0.05, A, None)
    c["sam_first_step null norm"] = lambda: lib.htrvt_sam_first_step(A, A, A, 8, 0.05, None, None)
    c["sam_restore n % 4"] = lambda: lib.htrvt_sam_restore(A, A, 6, None)
    c["sam_restore null p"] = lambda: lib.htrvt_sam_restore(None, A, 8, None)
    c["sam_restore null old"] = lambda: lib.htrvt_sam_restore(A, None, 8, None)
    return c


def test_every_glue_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    calls = _bad_calls(lib)
    assert len(calls) > 100
    for name, call in calls.items():
        _refused(lib, name, call)


def test_workspace_rule_and_empty_calls_need_no_gpu():
    lib = _lib()
    for rows in (1, 255, 256, 257, 8191, 8192, 8193, 12345):
        want = 0 if rows < 256 else min(rows // 128, 64) * 264
        assert lib.htrvt_colsum_workspace_floats(rows, 264) == want, rows
    # rows = 0: nothing to do, 0 before any buffer is looked at
    assert lib.htrvt_mask_tokens_fwd(None, None, 0, None, None, 0, 8, 1, None) == 0
    assert lib.htrvt_mask_tokens_bwd(None, None, 0, None, 0, 8, 1, None) == 0
