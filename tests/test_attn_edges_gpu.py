"""The fused bfloat16 attention kernels (csrc/attention_impl.h: forward, dQ, dK/dV; score sources of attention.hip and
attn_relpos.hip) through the C ABI, element by element, at ragged lengths and window edges.

Every expectation comes from tests/attn_refs.py and is proved on the host by tests/test_attn_refs_cpu.py: random cases are
held to C_GPU x the per-element error model around the float64 reference, the structured cases (one-hot, uniform windows,
window 1) to exact values.  Every output (out, lse2, delta, dqkv, dbias, dtable, the dtable workspace) is cut out of a
larger allocation, pre-filled with NaN (the accumulated ones with a known value) and its guard bands are compared
afterwards: a store one row past N shows.

Worst |got - ref| / error model measured on an MI355X over the random cases of this file (gate: C_GPU = 2.0):
    O 0.78, delta 0.57, dQ 0.47, dK 0.49, dV 0.91, dbias 0.44, dtable 0.19; lse2 within 1e-5 of float64
-- what the host emulation of attn_refs gives (0.80 / 0.58 / 0.47 / 0.52 / 0.91): the model lacks no rounding point."""
import pytest
import torch

import attn_refs as R

pytestmark = pytest.mark.gpu

BF16 = 1


def _abi():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import ptr, stream
    return lib, check, ptr, stream


def _plain_fwd(qkv, B, N, h, hd, bias=None):
    lib, check, ptr, stream = _abi()
    out = R.guarded((B * N, h * hd), torch.bfloat16)
    lse = R.guarded((B * h, N), torch.float32)
    check(lib.htrvt_attn_fwd(ptr(qkv), ptr(bias), ptr(out), ptr(lse), B, N, h, hd, hd ** -0.5, BF16, stream()), "attn_fwd")
    return out, lse


def _plain_bwd(qkv, out, dout, lse, B, N, h, hd, bias=None, dbias=None):
    lib, check, ptr, stream = _abi()
    dqkv = R.guarded((B * N, 3 * h * hd), torch.bfloat16)
    delta = R.guarded((B * h, N), torch.float32)
    check(lib.htrvt_attn_bwd(ptr(qkv), ptr(bias), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), ptr(dbias), B, N, h,
                             hd, hd ** -0.5, BF16, stream()), "attn_bwd")
    return dqkv, delta


def _table_fwd(qkv, table, B, N, h, hd, P, ws, shift):
    lib, check, ptr, stream = _abi()
    out = R.guarded((B * N, h * hd), torch.bfloat16)
    lse = R.guarded((B * h, N), torch.float32)
    check(lib.htrvt_attn_relpos_fwd(ptr(qkv), ptr(table), ptr(out), ptr(lse), B, N, h, hd, hd ** -0.5, P, ws, shift, BF16,
                                    stream()), "attn_relpos_fwd")
    return out, lse


def _table_bwd(qkv, table, out, dout, lse, B, N, h, hd, P, ws, shift, dtable_fill=0.0):
    """dtable_fill None: no table gradient and no workspace"""
    lib, check, ptr, stream = _abi()
    dqkv = R.guarded((B * N, 3 * h * hd), torch.bfloat16)
    delta = R.guarded((B * h, N), torch.float32)
    dtable = work = None
    if dtable_fill is not None:
        nwork = lib.htrvt_attn_relpos_bwd_workspace_floats(B, N, h, P, ws, shift)
        assert nwork == h * B * ((N + 127) // 128) * (2 * P - 1)
        dtable = R.guarded((2 * P - 1, h), torch.float32, fill=dtable_fill)
        work = R.guarded((nwork,), torch.float32)
    check(lib.htrvt_attn_relpos_bwd(ptr(qkv), ptr(table), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), ptr(dtable),
                                    ptr(work), B, N, h, hd, hd ** -0.5, P, ws, shift, BF16, stream()), "attn_relpos_bwd")
    return dqkv, delta, dtable


def _clean(*tensors):
    for t in tensors:
        assert not torch.isnan(t.float()).any(), "an element of an output was not written"


def _gate(name, got, want, bound):
    """per element: |got - want| <= C_GPU x bound"""
    ratio = R.worst_ratio(got.detach().cpu(), want, bound)
    print(f"RATIO {name} {ratio:.3f}")
    assert ratio <= R.C_GPU, (name, ratio)


def _gate_lse2(lse, want, B, h, N):
    err = float((lse.double().cpu().reshape(B, h, N) - want).abs().max())
    print(f"lse2 max-abs {err:.2e}")
    assert err < R.LSE2_TOL, err


def _gate_backward(dqkv, delta, ref, E, B, N, h, hd, want=None):
    """want: (dQ, dK, dV) when the values come from another reference than the error model's"""
    D = h * hd
    wq, wk, wv = (ref.dQ, ref.dK, ref.dV) if want is None else want
    _gate("delta", delta.reshape(B, h, N), ref.delta, E.delta)
    _gate("dQ", dqkv[:, :D], wq, E.dQ)
    _gate("dK", dqkv[:, D:2 * D], wk, E.dK)
    _gate("dV", dqkv[:, 2 * D:], wv, E.dV)


# ---- plain scores ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", R.PLAIN_HD)
@pytest.mark.parametrize("N", R.PLAIN_LENGTHS)
def test_plain_one_hot_forward_and_backward_are_exact(N, hd):
    B, h = R.one_hot_grid(N)
    c = R.one_hot_case(B, N, h, hd, 100 * N + hd)
    qkv, dout = c.qkv.cuda(), c.dout.cuda()
    out, lse = _plain_fwd(qkv, B, N, h, hd)
    dqkv, delta = _plain_bwd(qkv, out, dout, lse, B, N, h, hd)
    R.assert_guards_intact()
    _clean(out, lse, dqkv, delta)
    D = h * hd
    assert torch.equal(out.float().cpu(), c.O)
    assert torch.equal(dqkv[:, 2 * D:].float().cpu(), c.dV)
    assert float(dqkv[:, :2 * D].float().abs().max()) < 1e-5
    _gate_lse2(lse, R.attention_f64(c.qkv, B, N, h, hd).lse2, B, h, N)
    want_delta = (c.dout.double() * c.O.double()).reshape(B, N, h, hd).sum(-1).permute(0, 2, 1).reshape(B * h, N)
    assert torch.equal(delta.double().cpu(), want_delta)


@pytest.mark.parametrize("B,N,h,hd", R.PLAIN_RANDOM)
def test_plain_random_per_element(B, N, h, hd):
    qkv, dout, _, ref, E = R.plain_reference(B, N, h, hd)
    qd, dd = qkv.cuda(), dout.cuda()
    out, lse = _plain_fwd(qd, B, N, h, hd)
    dqkv, delta = _plain_bwd(qd, out, dd, lse, B, N, h, hd)
    R.assert_guards_intact()
    _clean(out, lse, dqkv, delta)
    _gate("O", out, ref.O, E.O)
    _gate_lse2(lse, ref.lse2, B, h, N)
    _gate_backward(dqkv, delta, ref, E, B, N, h, hd)


# ---- dense bias -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,h,hd", R.DENSE_RANDOM)
def test_dense_bias_per_element_and_bias_gradient(B, N, h, hd):
    qkv, dout, bias, ref, E = R.dense_reference(B, N, h, hd)
    masked = bias == R.MASKED
    assert bool(masked[:, 32:64, :64].all()) and bool((~masked).any(-1).all())      # a whole first tile; every query keeps a key
    qd, dd, bd = qkv.cuda(), dout.cuda(), bias.cuda()
    out, lse = _plain_fwd(qd, B, N, h, hd, bias=bd)
    db0 = R.guarded((h, N, N), torch.float32, fill=0.0)
    dqkv, delta = _plain_bwd(qd, out, dd, lse, B, N, h, hd, bias=bd, dbias=db0)
    db1 = R.guarded((h, N, N), torch.float32, fill=1.0)
    dqkv1, _ = _plain_bwd(qd, out, dd, lse, B, N, h, hd, bias=bd, dbias=db1)
    dqkv2, _ = _plain_bwd(qd, out, dd, lse, B, N, h, hd, bias=bd, dbias=None)        # a constant mask: no bias gradient
    R.assert_guards_intact()
    _clean(out, lse, dqkv, delta, db0, db1)
    _gate("O", out, ref.O, E.O)
    _gate_lse2(lse, ref.lse2, B, h, N)
    _gate_backward(dqkv, delta, ref, E, B, N, h, hd)
    _gate("dbias", db0, ref.dscore.sum(0), E.dbias)
    assert torch.equal(dqkv1, dqkv) and torch.equal(dqkv2, dqkv)
    # the accumulate rule: 1 + sum_b dscore.  The float32 additions (B into 1.0, in either order, and the B - 1 behind the
    # zero-filled run) each round by at most 2^-24 of a partial sum, none of which exceeds 1 + sum_b |dscore|
    db0c, db1c = db0.double().cpu(), db1.double().cpu()
    room = 2 * B * 2.0 ** -24 * (1.0 + 1.01 * ref.dscore.abs().sum(0))
    assert bool(((db1c - (1.0 + db0c)).abs() <= room).all())
    assert bool((db1.cpu()[masked] == 1.0).all()) and bool((db0.cpu()[masked] == 0.0).all())


# ---- table scores ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.TABLE_SWEEP)), ids=[str(c) for c in R.TABLE_SWEEP])
def test_table_sweep_per_element(i):
    lib = _abi()[0]
    N, ws, shift, P = R.TABLE_SWEEP[i]
    B, h, hd = R.TABLE_B, R.TABLE_H, R.table_hd(i)
    assert lib.htrvt_attn_relpos_supported(N, hd, BF16, P, ws, shift) == 1, lib.htrvt_last_error().decode()
    qkv, table, dout, ref, E, (idx, inside) = R.table_reference(i)
    w_o, w_dqkv, w_dt = R.windowed_reference_grads(qkv, table, dout, B, N, h, hd, P, ws, shift)
    qd, td, dd = qkv.cuda(), table.cuda(), dout.cuda()
    args = (B, N, h, hd, P, ws, shift)
    out, lse = _table_fwd(qd, td, *args)
    dqkv, delta, dt = _table_bwd(qd, td, out, dd, lse, *args, dtable_fill=0.0)
    out1, lse1 = _table_fwd(qd, td, *args)
    dqkv1, delta1, dt1 = _table_bwd(qd, td, out1, dd, lse1, *args, dtable_fill=1.0)
    dqkv2, _, _ = _table_bwd(qd, td, out, dd, lse, *args, dtable_fill=None)
    R.assert_guards_intact()
    _clean(out, lse, dqkv, delta, dt, dt1)
    D = h * hd
    _gate("O", out, w_o, E.O)
    _gate_lse2(lse, ref.lse2, B, h, N)
    _gate_backward(dqkv, delta, ref, E, B, N, h, hd, want=(w_dqkv[:, :D], w_dqkv[:, D:2 * D], w_dqkv[:, 2 * D:]))
    _gate("dtable", dt, w_dt, E.dtable)
    used = torch.zeros(2 * P - 1, dtype=torch.bool)
    used[idx[inside]] = True
    if (~used).any():
        assert float(dt.cpu()[~used].abs().max()) == 0.0
    # two runs bit for bit (no atomics), the table gradient is added to what dtable holds, and without it dqkv is the same
    assert torch.equal(out1, out) and torch.equal(lse1, lse) and torch.equal(dqkv1, dqkv) and torch.equal(delta1, delta)
    assert torch.equal(dt1, 1.0 + dt)
    assert torch.equal(dqkv2, dqkv)


@pytest.mark.parametrize("N,ws,shift", R.UNIFORM_WINDOW)
@pytest.mark.parametrize("hd", [64, 128])
def test_table_uniform_windows_are_exact(N, ws, shift, hd):
    B, h, P = 2, 2, N
    c = R.uniform_window_case(B, N, h, hd, P, ws, shift, 40 + N + shift)
    qd, td, dd = c.qkv.cuda(), c.table.cuda(), c.dout.cuda()
    args = (B, N, h, hd, P, ws, shift)
    out, lse = _table_fwd(qd, td, *args)
    dqkv, delta, dt = _table_bwd(qd, td, out, dd, lse, *args, dtable_fill=0.0)
    R.assert_guards_intact()
    _clean(out, lse, dqkv, delta, dt)
    D = h * hd
    assert torch.equal(out.double().cpu(), c.ref.O)
    assert torch.equal(delta.double().cpu().reshape(B, h, N), c.ref.delta)
    assert torch.equal(dqkv[:, 2 * D:].double().cpu(), c.ref.dV)
    assert float(dqkv[:, :2 * D].float().abs().max()) == 0.0
    assert torch.equal(dt.double().cpu(), c.dtable)          # a miscounted diagonal or wrap pair shows here
    _gate_lse2(lse, c.ref.lse2, B, h, N)


def test_table_window_one_is_exact():
    B, N, h, hd, P = 2, 257, 2, 64, 257
    c = R.window1_case(B, N, h, hd, P, 9)
    qd, td, dd = c.qkv.cuda(), c.table.cuda(), c.dout.cuda()
    args = (B, N, h, hd, P, 1, 0)
    out, lse = _table_fwd(qd, td, *args)
    dqkv, delta, dt = _table_bwd(qd, td, out, dd, lse, *args, dtable_fill=0.0)
    R.assert_guards_intact()
    _clean(out, lse, dqkv, delta, dt)
    D = h * hd
    assert torch.equal(out.float().cpu(), c.O)
    assert torch.equal(dqkv[:, 2 * D:].float().cpu(), c.dV)
    assert float(dqkv[:, :2 * D].float().abs().max()) == 0.0
    assert float(dt.abs().max()) == 0.0
    want_delta = (c.dout.double() * c.O.double()).reshape(B, N, h, hd).sum(-1).permute(0, 2, 1).reshape(B * h, N)
    assert torch.equal(delta.double().cpu(), want_delta)
    from attn_dropout_refs import table_bias
    _gate_lse2(lse, R.attention_f64(c.qkv, B, N, h, hd, bias=table_bias(c.table, N, P, 1, 0)).lse2, B, h, N)
