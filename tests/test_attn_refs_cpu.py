"""What tests/test_attn_edges_gpu.py expects of the fused attention kernels, proved on the host in float64 first
(tests/attn_refs.py): each exact construction's claim, the power-of-two window condition, the bfloat16 emulation within
1.0 x the error model on every random case the GPU file uses, the two windowed references against each other, the edges
the case lists must contain, and that the per-element gate rejects three small faults of which the suite's earlier aggregate
gates accept at least one."""
import pytest
import torch

import attn_dropout_refs as D
import attn_refs as R


def test_case_lists_contain_the_named_edges():
    assert set(R.PLAIN_LENGTHS) == {32, 33, 63, 64, 65, 127, 129, 191, 257, 521}
    assert {N for _, N, _, _ in R.PLAIN_RANDOM} == set(R.PLAIN_LENGTHS)
    for hd in R.PLAIN_HD:               # every head dim below one tile, between a tile and a block, and over several blocks
        mine = [N for _, N, _, d in R.PLAIN_RANDOM if d == hd]
        assert any(N < 64 for N in mine) and any(64 < N < 128 for N in mine) and any(N > 128 for N in mine), hd
    for N in (129, 191, 257, 521):      # the remapped grid (a multiple of 8 workgroups) and the plain one
        grids = [B * h * ((N + 127) // 128) % 8 == 0 for B, n, h, _ in R.PLAIN_RANDOM if n == N]
        assert True in grids and False in grids, N
    assert any(h == 3 for _, _, h, _ in R.PLAIN_RANDOM)
    assert all(B <= 2 and h <= 4 and N <= 521 for B, N, h, _ in R.PLAIN_RANDOM + R.DENSE_RANDOM)
    assert {N for _, N, _, _ in R.DENSE_RANDOM} == {128, 256, 384} and {d for _, _, _, d in R.DENSE_RANDOM} == {32, 64, 128}
    assert all(N % 128 == 0 for _, N, _, _ in R.DENSE_RANDOM)
    sweep = R.TABLE_SWEEP
    assert sweep == [(33, 0, 0, 33), (129, 0, 0, 200), (100, 12, 0, 100), (100, 12, 11, 128), (129, 16, 1, 129),
                     (200, 48, 5, 256), (200, 100, 99, 200), (321, 24, 23, 321), (321, 130, 0, 400), (520, 16, 8, 520),
                     (520, 3, 2, 520), (257, 1, 0, 257)]
    assert any(ws and 64 % ws for _, ws, _, _ in sweep) and any(ws > 128 for _, ws, _, _ in sweep)
    assert any(s == 1 for _, _, s, _ in sweep) and any(ws > 1 and s == ws - 1 for _, ws, s, _ in sweep)
    assert any(ws == 1 for _, ws, _, _ in sweep) and any(N > 256 for N, _, _, _ in sweep)
    assert {R.table_hd(i) for i in range(len(sweep))} == {64, 128}
    assert R.UNIFORM_WINDOW == [(200, 16, 0), (200, 16, 8), (96, 8, 1), (328, 16, 8), (520, 16, 8)]


def test_table_sweep_is_inside_the_written_geometry_rules():
    """check_geometry of csrc/attn_relpos.hip accepts every sweep case (its rules: N >= 32, N <= P <= 2048, 0 <= shift < ws,
    a shifted window needs two windows); the launch itself needs no device for this"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import lib
    for i, (N, ws, shift, P) in enumerate(R.TABLE_SWEEP):
        assert lib.htrvt_attn_relpos_supported(N, R.table_hd(i), 1, P, ws, shift) == 1, (N, ws, shift, P, lib.htrvt_last_error())
        assert lib.htrvt_attn_relpos_bwd_workspace_floats(R.TABLE_B, N, R.TABLE_H, P, ws, shift) == \
            R.TABLE_H * R.TABLE_B * ((N + 127) // 128) * (2 * P - 1)


@pytest.mark.parametrize("with_bias", [False, True])
def test_attention_f64_agrees_with_autograd(with_bias):
    B, N, h, hd = 2, 65, 3, 32
    qkv, dout = R.random_case(B, N, h, hd, 5)
    bias = None
    if with_bias:
        bias = (torch.randn(h, N, N, generator=torch.Generator().manual_seed(6)) * 0.5).double()
        bias[:, :, 7] = float("-inf")
        bias.requires_grad_(True)
    o, lse2, dqkv = D.attention_ref(qkv, B, N, h, hd, bias=bias, dout=dout)
    r = R.attention_f64(qkv, B, N, h, hd, bias=None if bias is None else bias.detach(), dout=dout)
    Dm = h * hd
    assert (r.O - o).abs().max() < 1e-12 and (r.lse2 - lse2).abs().max() < 1e-12
    for name, got, sl in (("dQ", r.dQ, slice(0, Dm)), ("dK", r.dK, slice(Dm, 2 * Dm)), ("dV", r.dV, slice(2 * Dm, 3 * Dm))):
        assert (got - dqkv[:, sl]).abs().max() < 1e-11, name
    assert (r.delta - (dout.double() * r.O).reshape(B, N, h, hd).sum(-1).permute(0, 2, 1)).abs().max() < 1e-12
    if with_bias:
        assert (r.dscore.sum(0) - bias.grad).abs().max() < 1e-11
        assert float(r.dscore[..., 7].abs().max()) == 0.0


@pytest.mark.parametrize("hd", R.PLAIN_HD)
@pytest.mark.parametrize("N", R.PLAIN_LENGTHS)
def test_one_hot_case_is_exact_in_float64(N, hd):
    B, h = R.one_hot_grid(N)
    c = R.one_hot_case(B, N, h, hd, 100 * N + hd)
    r = R.attention_f64(c.qkv, B, N, h, hd, dout=c.dout)
    onehot = torch.zeros_like(r.P).scatter_(-1, c.perm.unsqueeze(-1), 1.0)
    leak = float((r.P * (1 - onehot)).max())
    resid = max(float(r.dQ.abs().max()), float(r.dK.abs().max()))
    print(f"N={N} hd={hd}: leak {leak:.1e} dQ/dK residue {resid:.1e}")
    assert leak < 1e-38 and resid < 1e-30
    assert (r.O - c.O.double()).abs().max() < 1e-30 and (r.dV - c.dV.double()).abs().max() < 1e-30
    # the matched pair: dP == delta as integers once O is the stored (exact) value
    assert torch.equal(c.qkv.float().to(torch.bfloat16), c.qkv) and float(c.O.abs().max()) <= 8


@pytest.mark.parametrize("N,ws,shift", R.UNIFORM_WINDOW)
@pytest.mark.parametrize("hd", [64, 128])
def test_uniform_window_case_is_exact_in_float32(N, ws, shift, hd):
    B, h = 2, 2
    c = R.uniform_window_case(B, N, h, hd, N, ws, shift, 40 + N + shift)     # asserts the power-of-two condition
    counts = c.inside.sum(-1)
    assert bool(((counts & (counts - 1)) == 0).all())
    r = c.ref
    assert torch.equal(R.bf16(r.O), r.O) and torch.equal(R.bf16(r.dV), r.dV)
    assert torch.equal(r.delta.float().double(), r.delta)
    assert float(r.dQ.abs().max()) == 0.0 and float(r.dK.abs().max()) == 0.0
    t = r.dscore * 4096
    assert torch.equal(t, t.round())                                    # every term a multiple of 2^-12
    assert float(c.dtable_abs.max()) * 4096 < 2 ** 24                    # ... and every partial sum of an entry below 2^24 of them
    print(f"N={N} ws={ws} shift={shift} hd={hd}: max|dtable| {float(c.dtable.abs().max()):.1f}, sum of |terms| {float(c.dtable_abs.max()):.1f}")
    o, dqkv, dt = R.windowed_reference_grads(c.qkv, c.table, c.dout, B, N, h, hd, N, ws, shift)
    assert (o - r.O).abs().max() < 1e-12 and (dt - c.dtable).abs().max() < 1e-9
    assert (dqkv[:, 2 * h * hd:] - r.dV).abs().max() < 1e-12


def test_window1_case_is_exact():
    B, N, h, hd = 2, 257, 2, 64
    c = R.window1_case(B, N, h, hd, N, 9)
    o, dqkv, dt = R.windowed_reference_grads(c.qkv, c.table, c.dout, B, N, h, hd, N, 1, 0)
    Dm = h * hd
    assert torch.equal(o, c.O.double()) and torch.equal(dqkv[:, 2 * Dm:], c.dV.double())
    assert float(dqkv[:, :2 * Dm].abs().max()) == 0.0 and float(dt.abs().max()) == 0.0
    assert torch.equal(c.O.to(torch.bfloat16).float(), c.O)


def _emulation_ratios(qkv, dout, bias, ref, E, B, N, h, hd):
    em = R.emulate_bf16(qkv, B, N, h, hd, bias=bias, dout=dout)
    assert (em.lse2 - ref.lse2).abs().max() < R.LSE2_TOL
    return {n: R.worst_ratio(getattr(em, n), getattr(ref, n), getattr(E, n)) for n in ("O", "delta", "dQ", "dK", "dV", "dscore")}


def test_emulation_stays_within_the_error_model_on_every_random_case():
    worst = dict.fromkeys(("O", "delta", "dQ", "dK", "dV", "dscore"), 0.0)

    def take(tag, ratios):
        print(tag, " ".join(f"{n} {v:.2f}" for n, v in ratios.items()))
        for n, v in ratios.items():
            assert v <= 1.0, (tag, n, v)
            worst[n] = max(worst[n], v)

    for case in R.PLAIN_RANDOM:
        qkv, dout, _, ref, E = R.plain_reference(*case)
        take(f"plain {case}", _emulation_ratios(qkv, dout, None, ref, E, *case))
    for case in R.DENSE_RANDOM:
        qkv, dout, bias, ref, E = R.dense_reference(*case)
        take(f"dense {case}", _emulation_ratios(qkv, dout, bias, ref, E, *case))
    for i, (N, ws, shift, P) in enumerate(R.TABLE_SWEEP):
        qkv, table, dout, ref, E, _ = R.table_reference(i)
        bias = D.table_bias(table, N, P, ws, shift)
        take(f"table {R.TABLE_SWEEP[i]}", _emulation_ratios(qkv, dout, bias, ref, E, R.TABLE_B, N, R.TABLE_H, R.table_hd(i)))
    print("worst emulation / model:", worst)
    for n, v in worst.items():          # the figures the module docstring of attn_refs quotes
        assert v <= R.EMULATION_WORST[n] <= 1.0, (n, v)


@pytest.mark.parametrize("scale", [0.5, 3.0])
@pytest.mark.parametrize("N,hd", [(33, 32), (144, 64), (257, 128)])
def test_emulation_stays_within_the_error_model_at_other_input_scales(N, hd, scale):
    B, h = 1, 2
    qkv, dout = R.random_case(B, N, h, hd, 77 + N, scale=scale)
    ref = R.attention_f64(qkv, B, N, h, hd, dout=dout)
    ratios = _emulation_ratios(qkv, dout, None, ref, R.error_model(ref), B, N, h, hd)
    print(ratios)
    assert max(ratios.values()) <= 1.0


@pytest.mark.parametrize("i", range(len(R.TABLE_SWEEP)))
def test_the_two_windowed_references_agree(i):
    """the literal pad / roll / partition restatement against table_bias (variants.relative_position_index) + attention_f64"""
    N, ws, shift, P = R.TABLE_SWEEP[i]
    B, h, hd = R.TABLE_B, R.TABLE_H, R.table_hd(i)
    qkv, table, dout, ref, E, (idx, inside) = R.table_reference(i)
    o, dqkv, dt = R.windowed_reference_grads(qkv, table, dout, B, N, h, hd, P, ws, shift)
    Dm = h * hd
    assert (o - ref.O).abs().max() < 1e-11
    for name, got, sl in (("dQ", ref.dQ, slice(0, Dm)), ("dK", ref.dK, slice(Dm, 2 * Dm)), ("dV", ref.dV, slice(2 * Dm, 3 * Dm))):
        assert (got - dqkv[:, sl]).abs().max() < 1e-10, name
    assert (ref.dtable - dt).abs().max() < 1e-10
    used = torch.zeros(2 * P - 1, dtype=torch.bool)
    used[idx[inside]] = True
    assert float(dt[~used].abs().max() if (~used).any() else 0.0) == 0.0


def _accepts(got, want, bound):
    return R.worst_ratio(got, want, bound) <= R.C_GPU


def test_per_element_gate_rejects_what_the_aggregate_gates_let_through():
    """three small faults put into the float64 reference itself.  The per-element gate (C_GPU x error model) rejects each;
    the earlier gates (forward: max-abs < 2e-2; backward: max|err| / max|ref| < 2.5e-2 and cosine > 0.9995) accept at least
    one of them"""
    old = []
    # 1. ragged case N = 129 (last key tile = key 128 alone): two query rows lose that tile's contribution
    B, N, h, hd = 2, 129, 2, 64
    qkv, dout, _, ref, E = R.plain_reference(B, N, h, hd)
    p_last = ref.P[0, 0, :, 128].clone()
    # among the rows whose lost share stays below the old forward gate, the two that lose most
    lost = (ref.P[0, 0, :, 128:] @ ref.v[0, 0, 128:]).abs().max(-1).values
    rows = torch.argsort(torch.where(lost < 1.5e-2, lost, torch.zeros_like(lost)), descending=True)[:2]
    o = ref.o.clone()
    o[0, 0, rows] -= ref.P[0, 0, rows, 128:] @ ref.v[0, 0, 128:]
    bad = R.merge_heads(o)
    print(f"1. rows {rows.tolist()} P[., 128] = {p_last[rows].tolist()}: ratio {R.worst_ratio(bad, ref.O, E.O):.1f}")
    assert _accepts(ref.O, ref.O, E.O) and not _accepts(bad, ref.O, E.O)
    old.append(R.old_forward_gate(bad, ref.O))

    # 3. one dK row of the same case scaled by 1.1: a row of modest size, where a tenth is far from the largest value
    row_max = ref.dK.abs().max(-1).values
    ratio = (0.1 * ref.dK.abs() / E.dK).max(-1).values
    ok = row_max <= 0.2 * row_max.max()
    row = int(torch.argmax(torch.where(ok, ratio, torch.zeros_like(ratio))))
    bad = ref.dK.clone()
    bad[row] *= 1.1
    print(f"3. dK row {row}: ratio {R.worst_ratio(bad, ref.dK, E.dK):.1f}")
    assert not _accepts(bad, ref.dK, E.dK)
    old.append(R.old_backward_gate(bad, ref.dK))

    # 2. windowed case (200, 48, 5): one pair across the cyclic wrap (a token before the shift with one at the end) loses its
    # d(score) in the table gradient
    i = R.TABLE_SWEEP.index((200, 48, 5, 256))
    N, ws, shift, P = R.TABLE_SWEEP[i]
    qkv, table, dout, ref, E, (idx, inside) = R.table_reference(i)
    q = torch.arange(N)[:, None].expand(N, N)
    k = torch.arange(N)[None, :].expand(N, N)
    wrap = inside & ((q < shift) != (k < shift))
    assert wrap.any()
    cand = torch.where(wrap, ref.dscore[0, 0].abs(), torch.zeros(N, N, dtype=torch.float64))
    qq, kk = divmod(int(cand.argmax()), N)
    bad = ref.dtable.clone()
    bad[idx[qq, kk], 0] -= ref.dscore[0, 0, qq, kk]
    print(f"2. wrap pair ({qq}, {kk}) entry {int(idx[qq, kk])}: ratio {R.worst_ratio(bad, ref.dtable, E.dtable):.1f}")
    assert not _accepts(bad, ref.dtable, E.dtable)
    old.append(R.old_backward_gate(bad, ref.dtable))
    print("the earlier gates accept:", old)
    assert any(old)
