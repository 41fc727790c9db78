"""Dropout on the attention probabilities inside the fused kernels (csrc/attention_impl.h HashDrop: plain and table scores),
the same mask on the batched-GEMM route, and htrvt_residual_dropout -- against the numpy restatement of the mask and the
float64 attention of tests/attn_dropout_refs.py.

The mask is first pinned against the device-side oracle (htrvt_sgm_dropout on a ones tensor), then recovered EXACTLY from
the kernels: with q = 0 every probability is 1/N, and with one-hot V / dO rows `out N (1 - p)` and `dV N (1 - p)` are integer
counts of kept pairs per residue class -- a transposed, shifted or per-tile-restarted mask index is off by O(1).  Random
data then checks the arithmetic at the gates of the p = 0 tests (tests/test_attention_gpu.py, test_attn_relpos_gpu.py)
times 1 / (1 - p): the bf16 rounding of P M / (1 - p) and of dS scales by exactly that factor."""
import numpy as np
import pytest
import torch

import attn_dropout_refs as R

pytestmark = pytest.mark.gpu

# (B, N, h, hd): one partial tile; a ragged last key tile; two query blocks with an odd head count (a wrong b h + head
# shows); both dK/dV query-tile sizes (128 at hd 64, 64 at hd 128) with more than one staged tile; hd 32
PLAIN = [(2, 32, 2, 128), (2, 96, 2, 64), (1, 160, 3, 128), (2, 256, 2, 64), (1, 256, 2, 128), (1, 72, 2, 32),
         (2, 65, 2, 64), (1, 129, 3, 128)]      # odd lengths: the mask index has stride N
TABLE = [(64, 64, 0, 0), (200, 128, 16, 8), (256, 64, 16, 0)]         # (N, hd, ws, shift) at P = 256, B = 2, h = 2
TB, TH, TP = 2, 2, 256
BF = 1
SEED = 0x1234_5678_9ABC_DEF                                             # below 2^62, above 2^32


def _env():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import ptr, stream
    return seq_ops, lib, check, ptr, stream


def _seed(v=SEED):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def _plain(qkv, dout, B, N, h, p, seed):
    """forward + backward through seq_ops -> (out, lse, dqkv)"""
    S = _env()[0]
    drop = None if p is None else (_seed(seed), p)
    out, lse = S.attention_fwd(qkv, B, N, h, drop=drop)
    dqkv = None if dout is None else S.attention_bwd(qkv, out, dout, lse, B, N, h, drop=drop)
    torch.cuda.synchronize()
    return out, lse, dqkv


def _table(qkv, table, dout, N, ws, shift, p, seed):
    """-> (out, lse, dqkv, dtable)"""
    S = _env()[0]
    drop = None if p is None else (_seed(seed), p)
    out, lse = S.relpos_attention_fwd(qkv, table, TB, N, TH, TP, ws, shift, drop=drop)
    if dout is None:
        return out, lse, None, None
    dtable = torch.zeros_like(table)
    dqkv = S.relpos_attention_bwd(qkv, table, out, dout, lse, TB, N, TH, TP, ws, shift, dtable=dtable, drop=drop)
    torch.cuda.synchronize()
    return out, lse, dqkv, dtable


def _rand(B, N, h, hd, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * N, 3 * h * hd, generator=g) * 1.2).to(torch.bfloat16)
    dout = torch.randn(B * N, h * hd, generator=g).to(torch.bfloat16)
    return qkv, dout


def _gate(name, got, want, tol, cos_min=0.9995):
    got = got.double().cpu()
    e = (got - want).abs().max().item() / want.abs().max().item()
    cos = float((got.flatten() @ want.flatten()) / (got.norm() * want.norm()))
    print(f"   {name}: rel-to-max {e:.3e} (gate {tol:.3e}) cosine {cos:.6f}")
    assert e < tol and cos > cos_min, (name, e, cos)


# ---- the mask -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,h,hd", PLAIN)
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_mask_oracle_sgm_dropout_on_ones_is_the_restated_mask(B, N, h, hd, p):
    S = _env()[0]
    # the mask is a function of the flat element index, and htrvt_sgm_dropout takes whole groups of 8 elements: at an odd N
    # the flat tensor is drawn a few elements longer and cut
    n = B * h * N * N
    n8 = (n + 7) // 8 * 8
    y = S.dropout(torch.ones(n8, device="cuda"), _seed(), p)[:n]
    want = R.keep_mask(SEED, B, h, N, p)
    assert np.array_equal(y.cpu().numpy().reshape(B, h, N, N) != 0, want)
    assert set(np.unique(y.cpu().numpy()).tolist()) <= {0.0, R.scale_of(p)}
    yb = S.dropout(torch.ones(n8, device="cuda", dtype=torch.bfloat16), _seed(), p)[:n]
    assert np.array_equal(yb.float().cpu().numpy().reshape(B, h, N, N) != 0, want)


def _one_hot_rows(B, N, h, hd):
    """[B, N, h, hd] with row n = unit vector n mod hd"""
    e = torch.zeros(N, hd)
    e[torch.arange(N), torch.arange(N) % hd] = 1.0
    return e[None, :, None, :].expand(B, N, h, hd)


def _counts(keep, N, hd, over):
    """keep [B, h, N(q), N(k)] -> integer counts per residue class d of the axis `over` ('k': [B,h,q,d], 'q': [B,h,k,d])"""
    cls = torch.nn.functional.one_hot(torch.arange(N) % hd, hd).double()      # [N, hd]
    kp = torch.as_tensor(keep).double()
    return kp @ cls if over == "k" else kp.transpose(-1, -2) @ cls


def _recovery_inputs(B, N, h, hd):
    qkv = torch.zeros(B, N, 3, h, hd)
    qkv[:, :, 2] = _one_hot_rows(B, N, h, hd)                          # V[k][d] = [d == k mod hd]; q = k = 0: P = 1/N
    dout = _one_hot_rows(B, N, h, hd)                                  # dO[q][d] = [d == q mod hd]
    return (qkv.reshape(B * N, 3 * h * hd).to(torch.bfloat16).cuda(), dout.reshape(B * N, h * hd).to(torch.bfloat16).cuda())


def _check_recovery(out, dqkv, B, N, h, hd, p):
    keep = R.keep_mask(SEED, B, h, N, p)
    got = out.double().cpu().reshape(B, N, h, hd).permute(0, 2, 1, 3) * N * (1 - p)           # [B,h,q,d]
    want = _counts(keep, N, hd, "k")
    err = (got - want).abs().max().item()
    print(f"   forward: counts up to {int(want.max())}, worst deviation {err:.4f}")
    assert err < 0.1
    dv = dqkv.double().cpu().reshape(B, N, 3, h, hd)[:, :, 2].permute(0, 2, 1, 3) * N * (1 - p)   # [B,h,k,d]
    want = _counts(keep, N, hd, "q")
    err = (dv - want).abs().max().item()
    print(f"   dV: counts up to {int(want.max())}, worst deviation {err:.4f}")
    assert err < 0.1


@pytest.mark.parametrize("B,N,h,hd", PLAIN)
def test_exact_mask_recovery_plain_scores(B, N, h, hd):
    """forward: out[q][d] N (1 - p) = #{k = d mod hd : keep(q, k)}; dK/dV launch (lanes own keys, registers are queries):
    dV[k][d] N (1 - p) = #{q = d mod hd : keep(q, k)}"""
    p = 0.5
    qkv, dout = _recovery_inputs(B, N, h, hd)
    out, _, dqkv = _plain(qkv, dout, B, N, h, p, SEED)
    _check_recovery(out, dqkv, B, N, h, hd, p)


def test_exact_mask_recovery_table_scores():
    N, hd, ws, shift = TABLE[0]
    assert ws == 0
    p = 0.5
    qkv, dout = _recovery_inputs(TB, N, TH, hd)
    table = torch.zeros(2 * TP - 1, TH, device="cuda")
    out, _, dqkv, _ = _table(qkv, table, dout, N, ws, shift, p, SEED)
    _check_recovery(out, dqkv, TB, N, TH, hd, p)


# ---- random data against float64 with the restated mask ---------------------------------------------------------------------

@pytest.mark.parametrize("B,N,h,hd", PLAIN)
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_plain_scores_random_against_float64(B, N, h, hd, p):
    qkv, dout = _rand(B, N, h, hd, 11 * N + hd)
    keep = R.keep_mask(SEED, B, h, N, p)
    ref_o, ref_lse, ref_d = R.attention_ref(qkv, B, N, h, hd, keep=keep, p=p, dout=dout)
    out, lse, dqkv = _plain(qkv.cuda(), dout.cuda(), B, N, h, p, SEED)
    s = 1.0 / (1.0 - p)
    err = (out.double().cpu() - ref_o).abs().max().item()
    lerr = (lse.double().cpu().reshape(B, h, N) - ref_lse).abs().max().item()
    print(f"\nN={N} hd={hd} p={p}: out max-abs {err:.3e} (gate {2e-2 * s:.3e}), lse2 {lerr:.3e}")
    assert not torch.isnan(dqkv.float()).any()
    assert err < 2e-2 * s
    assert lerr < 2e-3                                                  # dropout must not change lse2
    D = h * hd
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        _gate(name, dqkv[:, sl], ref_d[:, sl], 2.5e-2 * s)


@pytest.mark.parametrize("N,hd,ws,shift", TABLE, ids=lambda v: str(v))
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_table_scores_random_against_float64(N, hd, ws, shift, p):
    g = torch.Generator().manual_seed(100 + N + hd + ws + shift)
    D = TH * hd
    qkv = torch.randn(TB * N, 3 * D, generator=g).to(torch.bfloat16)
    table = torch.randn(2 * TP - 1, TH, generator=g) * 0.5
    dout = torch.randn(TB * N, D, generator=g).to(torch.bfloat16)
    keep = R.keep_mask(SEED, TB, TH, N, p)
    tr = table.double().clone().requires_grad_(True)
    ref_o, ref_lse, ref_d = R.attention_ref(qkv, TB, N, TH, hd, keep=keep, p=p, bias=R.table_bias(tr, N, TP, ws, shift), dout=dout)
    out, lse, dqkv, dtable = _table(qkv.cuda(), table.cuda(), dout.cuda(), N, ws, shift, p, SEED)
    s = 1.0 / (1.0 - p)
    err = (out.double().cpu() - ref_o).abs().max().item()
    lerr = (lse.double().cpu().reshape(TB, TH, N) - ref_lse).abs().max().item()
    print(f"\nN={N} hd={hd} ws={ws} shift={shift} p={p}: out max-abs {err:.3e} (gate {2.5e-2 * s:.3e}), lse2 {lerr:.3e}")
    assert err < 2.5e-2 * s
    assert lerr < 2e-3
    _gate("dqkv", dqkv, ref_d, 3e-2 * s)
    _gate("dtable", dtable, tr.grad, 3e-2 * s)


# ---- bitwise properties -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,h,hd", [PLAIN[1], PLAIN[4]])
def test_plain_p_zero_is_the_existing_entry_point_and_seeds_are_honoured(B, N, h, hd):
    _, lib, check, ptr, stream = _env()
    qkv, dout = [t.cuda() for t in _rand(B, N, h, hd, 5 + N)]
    o0, l0, d0 = _plain(qkv, dout, B, N, h, None, SEED)
    out = torch.empty_like(o0)
    lse, delta, dqkv = torch.empty_like(l0), torch.empty_like(l0), torch.empty_like(d0)
    sc = hd ** -0.5
    check(lib.htrvt_attn_dropout_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, h, hd, sc, None, 0.0, BF, stream()), "fwd")     # seed NULL
    check(lib.htrvt_attn_dropout_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), B, N, h, hd, sc, None, 0.0,
                                     BF, stream()), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(out, o0) and torch.equal(lse, l0) and torch.equal(dqkv, d0)
    a = _plain(qkv, dout, B, N, h, 0.5, SEED)
    b = _plain(qkv, dout, B, N, h, 0.5, SEED)
    c = _plain(qkv, dout, B, N, h, 0.5, SEED + 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[1], l0) and torch.equal(c[1], l0)             # lse2 is that of the undropped softmax, bitwise
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2])
    assert not torch.equal(a[0], o0)


@pytest.mark.parametrize("N,hd,ws,shift", [TABLE[1]], ids=lambda v: str(v))
def test_table_p_zero_is_the_existing_entry_point_and_seeds_are_honoured(N, hd, ws, shift):
    _, lib, check, ptr, stream = _env()
    S = _env()[0]
    g = torch.Generator().manual_seed(3)
    D = TH * hd
    qkv = torch.randn(TB * N, 3 * D, generator=g).to(torch.bfloat16).cuda()
    table = (torch.randn(2 * TP - 1, TH, generator=g) * 0.5).cuda()
    dout = torch.randn(TB * N, D, generator=g).to(torch.bfloat16).cuda()
    o0, l0, d0, t0 = _table(qkv, table, dout, N, ws, shift, None, SEED)
    out = torch.empty_like(o0)
    lse, delta, dqkv, dtable = torch.empty_like(l0), torch.empty_like(l0), torch.empty_like(d0), torch.zeros_like(t0)
    work = torch.empty(S.relpos_workspace_floats(TB, N, TH, TP, ws, shift), device="cuda")
    sc = hd ** -0.5
    check(lib.htrvt_attn_relpos_dropout_fwd(ptr(qkv), ptr(table), ptr(out), ptr(lse), TB, N, TH, hd, sc, TP, ws, shift, None, 0.0,
                                            BF, stream()), "fwd")
    check(lib.htrvt_attn_relpos_dropout_bwd(ptr(qkv), ptr(table), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv),
                                            ptr(dtable), ptr(work), TB, N, TH, hd, sc, TP, ws, shift, None, 0.0, BF, stream()),
          "bwd")
    torch.cuda.synchronize()
    assert torch.equal(out, o0) and torch.equal(lse, l0) and torch.equal(dqkv, d0) and torch.equal(dtable, t0)
    a = _table(qkv, table, dout, N, ws, shift, 0.5, SEED)
    b = _table(qkv, table, dout, N, ws, shift, 0.5, SEED)
    c = _table(qkv, table, dout, N, ws, shift, 0.5, SEED + 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[1], l0)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2]) and not torch.equal(a[3], c[3])


def test_a_missing_seed_with_dropout_is_refused():
    _, lib, _, ptr, stream = _env()
    x = torch.zeros(64, 3 * 64, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    assert lib.htrvt_attn_dropout_fwd(ptr(x), ptr(o), None, 1, 64, 1, 64, 0.125, None, 0.1, BF, stream()) != 0
    assert "null" in lib.htrvt_last_error().decode()


# ---- the same mask on both routes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ws,shift", [(0, 0), (16, 0)])
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_fused_bf16_and_unfused_float32_share_the_mask(ws, shift, p):
    """variants.relpos_self_attention with one seed: bfloat16 on the fused table kernels, float32 on the dense bias +
    batched GEMMs + htrvt_sgm_dropout on P / dP (N = 128 is a multiple of 8: both index the mask at N).  Gate: that of
    test_relpos_agrees_with_dense_bias_route times 1 / (1 - p)."""
    from htrvt_amd import variants as V
    B, N, h, hd, P = 3, 128, 6, 128, 256
    g = torch.Generator().manual_seed(7 + N + ws)
    D = h * hd
    qkv = torch.randn(B * N, 3 * D, generator=g).to(torch.bfloat16)
    table = torch.randn(2 * P - 1, h, generator=g) * 0.5
    dout = torch.randn(B * N, D, generator=g).to(torch.bfloat16)
    res = []
    for dtype in (torch.bfloat16, torch.float32):
        qd = qkv.to(dtype).cuda().requires_grad_(True)
        td = table.cuda().requires_grad_(True)
        out = V.relpos_self_attention(qd, td, B, N, h, P, ws, shift, dropout_p=p, seed=_seed())
        out.backward(dout.to(dtype).cuda())
        torch.cuda.synchronize()
        res.append((out.detach(), qd.grad, td.grad))
    s = 1.0 / (1.0 - p)
    (o1, q1, t1), (o2, q2, t2) = res
    _gate("out", o1, o2.double().cpu(), tol=2e-2 * s, cos_min=0.9999)
    _gate("dqkv", q1, q2.double().cpu(), tol=2e-2 * s, cos_min=0.9999)
    _gate("dtable", t1, t2.double().cpu(), tol=1e-2 * s, cos_min=0.99999)


def test_self_attention_wrapper_routes_and_draws_a_seed():
    """variants.self_attention: bfloat16 fused and float32 unfused agree for one seed; seed=None draws one from the CUDA
    generator (reproducible under torch.cuda.manual_seed, different from one call to the next)"""
    from htrvt_amd import variants as V
    B, N, h, hd, p = 2, 96, 2, 64, 0.5
    qkv, dout = _rand(B, N, h, hd, 17)
    res = []
    for dtype in (torch.bfloat16, torch.float32):
        qd = qkv.to(dtype).cuda().requires_grad_(True)
        out = V.self_attention(qd, B, N, h, dropout_p=p, seed=_seed())
        out.backward(dout.to(dtype).cuda())
        res.append((out.detach(), qd.grad))
    keep = R.keep_mask(SEED, B, h, N, p)
    ref_o, _, ref_d = R.attention_ref(qkv, B, N, h, hd, keep=keep, p=p, dout=dout)
    _gate("float32 out", res[1][0], ref_o, 1e-4, 0.999999)             # the float32 gates of test_attn_relpos_gpu.py
    _gate("float32 dqkv", res[1][1], ref_d, 1e-4, 0.999999)
    assert (res[0][0].double().cpu() - ref_o).abs().max().item() < 2e-2 / (1 - p)
    _gate("bf16 dqkv", res[0][1], ref_d, 2.5e-2 / (1 - p))
    qd = qkv.cuda()
    torch.cuda.manual_seed(5)
    a = V.self_attention(qd, B, N, h, dropout_p=p)
    b = V.self_attention(qd, B, N, h, dropout_p=p)
    torch.cuda.manual_seed(5)
    c = V.self_attention(qd, B, N, h, dropout_p=p)
    assert torch.equal(a, c) and not torch.equal(a, b)
    o0, _, _ = _plain(qd, None, B, N, h, None, SEED)
    assert torch.equal(V.self_attention(qd, B, N, h), o0)              # dropout_p = 0: the existing launch


# ---- residual + drop_path(dropout(x)) ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,rows,D", [(3, 33, 64), (2, 5, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_residual_dropout(B, rows, D, dtype):
    """every element is res or res + x s, s = 1 / (1 - p) / (1 - p_path), by the restated masks; a sample is dropped as a
    whole; the backward uses the same masks.  Allowance, in float64: the kernel rounds s to float32 (2^-24 relative), the
    product x s and the sum once each in float32, and the result to the element type: eps (|x s| + |y|) with eps = 2^-22
    (float32) / 2^-8 (bfloat16: one rounding to 8 bits, 2^-9, doubled)."""
    from htrvt_amd import variants as V
    p, pp = 0.1, 0.4
    g = torch.Generator().manual_seed(B * rows + D)
    x = torch.randn(B * rows, D, generator=g).to(dtype)
    res = torch.randn(B * rows, D, generator=g).to(dtype)
    dy = torch.randn(B * rows, D, generator=g).to(dtype)
    seeds = torch.tensor([SEED, SEED + 77], dtype=torch.int64, device="cuda")
    keep_e = torch.as_tensor(R.keep_elems(SEED, np.arange(B * rows * D), p).reshape(B * rows, D)).double()
    for s1 in range(64):                                                # a seed that drops some sample but not all
        keep_s = R.keep_elems(SEED + 77 + s1, np.arange(B), pp)
        if 0 < keep_s.sum() < B:
            break
    seeds[1] += s1
    keep_s = torch.as_tensor(keep_s).double().repeat_interleave(rows)[:, None]
    s = 1.0 / (1.0 - p) / (1.0 - pp)
    eps = 2.0 ** -22 if dtype == torch.float32 else 2.0 ** -8

    xd, rd = x.cuda().requires_grad_(True), res.cuda().requires_grad_(True)
    y = V.residual_dropout(xd, rd, B, p, pp, seeds)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    branch = x.double() * keep_e * keep_s * s
    want = res.double() + branch
    got = y.detach().double().cpu()
    assert bool(((got - want).abs() <= eps * (branch.abs() + want.abs())).all())
    dropped = keep_s.expand_as(got) == 0
    assert dropped.any() and torch.equal(y.detach().cpu()[dropped], res[dropped])       # a dropped sample is res, bitwise
    dwant = dy.double() * keep_e * keep_s * s
    dgot = xd.grad.double().cpu()
    assert bool(((dgot - dwant).abs() <= eps * 2 * dwant.abs()).all())
    assert torch.equal(rd.grad.cpu(), dy)
    assert torch.equal(V.residual_dropout(xd, rd, B, p, pp, seeds).detach(), y.detach())

    y0 = V.residual_dropout(x.cuda(), res.cuda(), B, 0.0, 0.0)          # no seeds needed
    assert torch.equal(y0.cpu(), res + x)
    only_path = V.residual_dropout(x.cuda(), res.cuda(), B, 0.0, pp, seeds).double().cpu()
    wp = res.double() + x.double() * keep_s / (1.0 - pp)
    assert bool(((only_path - wp).abs() <= eps * ((x.double() * keep_s / (1 - pp)).abs() + wp.abs())).all())
