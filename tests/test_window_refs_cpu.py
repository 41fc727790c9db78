"""What tests/test_window_edges_gpu.py expects of the window and neighbourhood attention kernels (csrc/window_attn_impl.h with
lgp.hip, swin.hip, svtr.hip), proved on the host first (tests/window_refs.py): the dense forms against the references the
suite already trusts (1e-12 of the maximum), the exact constructions' claims, the bfloat16 emulation within 1.0 x the error
model on every random case the GPU file uses, and six injected faults that the per-element gate rejects.

Worst |emulation - float64| / model over the random cases (window_refs.EMULATION_WORST holds the ceilings asserted here):
    1-D local    out 0.81, dqkv 0.92, dpad 0.91
    2-D windows  out 0.84, dqkv 0.95, dtable 0.14
    boxes        out 0.76, dqkv 0.87, lse 0.15

The injected faults, all rejected by the per-element gate in both dtypes, and what the older aggregate gates of the four GPU
files say to them (forward: max-abs < 2.5e-2 bfloat16 / 2e-5 float32; gradients: 3e-2 / 1e-4 of the maximum with cosine >
0.9995 / 0.999999) -- OLD_GATES below, asserted:
    1. the padding key of a ragged 1-D window masked instead of attended      bfloat16 rejects, float32 rejects
    2. the wrap slot of a shifted window reading the token before its own     bfloat16 rejects, float32 rejects
    3. a key one column outside a clipped box, as a zero row (one query)      bfloat16 rejects (3 x 5 box; ACCEPTS at 7 x 11), float32 rejects
    4. the -100 mask applied as -inf (swin_refs.pinned_mask_case)             bfloat16 rejects, float32 rejects
    5. the corner entry (wh - 1, ww - 1) of dtable dropped                    bfloat16 ACCEPTS, float32 rejects
    6. an odd window's weight-0 partner row counted once more in dv           bfloat16 rejects, float32 rejects
The float32 aggregate gates are tight enough for whole-row faults; what they cannot see is an error of a few float32 ulps of
the tensor's maximum in one small element, which is what the E32 rule is for (fault 5 scaled to one window shows it below)."""
import math

import pytest
import torch

import svtr_refs as SV
import swin_refs as SR
import window_refs as R
from window_refs import BF, F32, F64

OLD_GATES = {1: (False, False), 2: (False, False), 3: (False, False), 4: (False, False), 5: (True, False), 6: (False, False)}


def _close(name, got, want, tol=1e-12):
    e = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
    assert e < tol, (name, e)


# ---- the lists -----------------------------------------------------------------------------------------------------------
def test_case_lists_contain_the_named_edges():
    L = R.LOCAL_CASES
    assert {w for _, _, _, w, _ in L} == {1, 2, 12, 15, 16}
    for w in (2, 12, 15, 16):
        mine = [(N, s) for _, N, _, ww, s in L if ww == w]
        assert any(N < w for N, _ in mine) and any(N % w == 1 for N, _ in mine) and any(N % w == w - 1 for N, _ in mine), w
        assert any(N % w == 0 for N, _ in mine), w
        assert any(s == w - 1 and N % w for N, s in mine) and any(s == 1 and N % w for N, s in mine) or w == 2, w
    assert any(N == 1 for _, N, _, _, _ in L) and any(s is not None and s == N - 1 and N % w for _, N, _, w, s in L)
    units = {R.local_units(B, N, h, w) for B, N, h, w, _ in L}
    assert 1 in units and any(u % 2 for u in units if u > 1) and any(u % 4 == 2 for u in units) and any(u % 4 == 0 for u in units)
    assert all(s is None or 0 <= s < w for _, _, _, w, s in L)
    Wn = R.WIN2D_CASES
    assert {(wh, ww) for *_, wh, ww, _, _ in Wn} >= {(4, 8), (2, 16), (1, 32), (3, 5), (3, 3), (5, 5), (1, 1)}
    assert {hd for _, _, _, _, hd, *_ in Wn} == {32, 64, 128} and {h for _, _, _, h, *_ in Wn} >= {1, 6}
    assert any(sh == wh - 1 and sw == ww - 1 and wh > 1 and ww > 1 for *_, wh, ww, sh, sw in Wn)
    assert any(sh == 0 and sw > 0 for *_, sh, sw in Wn) and any(sh > 0 and sw == 0 for *_, sh, sw in Wn)
    assert any(H == wh and sh > 0 for _, H, _, _, _, wh, _, sh, _ in Wn)
    items = [R.form_win2d(*c).items for c in Wn]
    assert any(i < 4 for i in items) and 256 in items and any(i > 256 and i % 256 for i in items)
    Nb = R.NBR2D_CASES
    assert {H for _, H, *_ in Nb} >= {1, 4, 5, 8, 9, 12, 16} and {W for _, _, W, *_ in Nb} >= {1, 15, 16, 17, 33}
    assert {(kh, kw) for *_, kh, kw in Nb} == {(1, 1), (7, 11), (7, 1), (1, 11), (3, 5)} and {c[4] for c in Nb} == {32, 64}
    assert any(H <= kh // 2 and W <= kw // 2 for _, H, W, _, _, kh, kw in Nb) and any(B >= 40 and H < 4 and W < 16 for B, H, W, *_ in Nb)
    assert [R.nbr2d_tile_rows(32, BF, H) for H in (1, 4, 5, 8, 9, 12, 16)] == [4, 4, 8, 8, 4, 4, 8]


# ---- the dense forms against the references the suite already trusts -----------------------------------------------------
@pytest.mark.parametrize("case", R.LOCAL_FULL[::2] + R.LOCAL_FULL[1:6:2], ids=str)
def test_local_dense_form_is_the_forks_window_attention(case):
    B, N, h, hd, w, shift = case
    D = h * hd
    qkv, bias, dout = R.random_inputs("local", case, F32)
    qr, br = qkv.double().requires_grad_(True), bias.double().requires_grad_(True)
    o = R.ref_local(qr, br, B, N, h, hd, w) if shift is None else R.ref_shifted(qr, br, B, N, h, hd, w, shift)
    o.backward(dout.double())
    _, ref = R.reference(R.make_form("local", case), qkv, bias, dout)
    _close("out", ref.out, o.detach())
    _close("dqkv", ref.dqkv, qr.grad)
    if N % w:
        assert float(br.grad[:D].abs().max()) == 0.0
        _close("dpad", ref.dpad.sum(0), br.grad[D:])
        for b in range(B):          # per image: the gradient of that image's rows alone
            qb, bb = qkv.double()[b * N:(b + 1) * N].requires_grad_(True), bias.double().requires_grad_(True)
            ob = R.ref_local(qb, bb, 1, N, h, hd, w) if shift is None else R.ref_shifted(qb, bb, 1, N, h, hd, w, shift)
            ob.backward(dout.double()[b * N:(b + 1) * N])
            _close("dpad[b]", ref.dpad[b], bb.grad[D:])
    else:
        assert float(ref.dpad.abs().max()) == 0.0 and (br.grad is None or float(br.grad.abs().max()) == 0.0)


@pytest.mark.parametrize("case", R.WIN2D_CASES, ids=str)
def test_win2d_dense_form_is_swin_refs(case):
    B, H, W, h, hd, wh, ww, sh, sw = case
    qkv, table, dout = R.random_inputs("win2d", case, F32)
    o, dqkv, dtable = SR.win2d_grads(qkv.double(), table.double(), dout.double(), B, H, W, h, (wh, ww), (sh, sw))
    _, ref = R.reference(R.make_form("win2d", case), qkv, table, dout)
    _close("out", ref.out, o)
    _close("dqkv", ref.dqkv, dqkv)
    _close("dtable", ref.dtable, dtable)


@pytest.mark.parametrize("case", R.NBR2D_CASES, ids=str)
def test_nbr2d_dense_form_is_svtr_refs(case):
    B, H, W, h, hd, kh, kw = case
    qkv, _, dout = R.random_inputs("nbr2d", case, F32)
    o, dqkv = SV.nbr2d_grads(qkv.double(), dout.double(), B, H, W, h, (kh, kw))
    _, ref = R.reference(R.make_form("nbr2d", case), qkv, None, dout)
    _close("out", ref.out, o)
    _close("dqkv", ref.dqkv, dqkv)
    q, k, _ = [t.transpose(1, 2) for t in qkv.double().view(B, H * W, 3, h, hd).unbind(2)]
    S = (q @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(~SV.visible(H, W, (kh, kw)), float("-inf"))
    _close("lse", ref.lse, S.logsumexp(-1).reshape(B * h, H * W))


# ---- the emulation inside the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_emulation_stays_within_the_error_model_on_every_random_case(family):
    worst = dict.fromkeys(R.OUTPUTS[family], 0.0)
    for case in R.FAMILIES[family]:
        c = R.case_reference(family, case, BF)
        em = vars(R.emulate_bf16(c.form, c.qkv, c.side, c.dout))
        ratios = {n: R.worst_ratio(em[n], c.ref[n], c.bound[n]) for n in R.OUTPUTS[family]}
        print(family, case, " ".join(f"{n} {v:.2f}" for n, v in ratios.items()))
        for n, v in ratios.items():
            assert v <= 1.0, (family, case, n, v)
            worst[n] = max(worst[n], v)
    print("worst emulation / model:", family, worst)
    for n, v in worst.items():          # the figures the module docstrings quote
        assert v <= R.EMULATION_WORST[family][n] <= 1.0, (family, n, v)


def test_float32_floor_is_the_projects_rule():
    """8 x the float32 evaluation error of the reference on the case's own inputs x the output's maximum: a few 1e-7 of it"""
    c = R.case_reference("win2d", R.WIN2D_CASES[3], F32)
    for n in R.OUTPUTS["win2d"]:
        rel = c.floor[n] / float(c.ref[n].abs().max())
        print(n, f"{rel:.2e}")
        assert 1e-8 < rel < 2e-5 and torch.equal(c.bound[n], torch.full_like(c.ref[n], c.floor[n]))


# ---- the exact constructions ---------------------------------------------------------------------------------------------
PROBES = [("local", (1, 14, 1, 64, 15, 13), 13), ("local", (2, 20, 3, 64, 12, 11), 8), ("local", (1, 100, 1, 128, 12, None), 99),
          ("win2d", (1, 4, 8, 1, 32, 4, 8, 3, 7), 0), ("win2d", (3, 8, 16, 1, 32, 4, 8, 2, 4), 127), ("win2d", (2, 6, 10, 1, 64, 3, 5, 2, 0), 24),
          ("nbr2d", (2, 4, 15, 2, 32, 7, 11), 0), ("nbr2d", (1, 16, 17, 1, 32, 7, 11), 16 * 17 - 1), ("nbr2d", (1, 9, 33, 1, 32, 1, 11), 4 * 33 + 16)]


@pytest.mark.parametrize("family,case,t0", PROBES, ids=str)
def test_membership_probe_is_one_over_n_on_the_key_set_and_zero_elsewhere(family, case, t0):
    form = R.make_form(family, case)
    p = R.membership_probe(form, t0, 3, F32)
    r, ref = R.reference(form, p.qkv, p.side)
    col = ref.out[:form.N, 3]
    assert (col[p.member] - 1.0 / p.n[p.member]).abs().max() < 1e-15
    assert float(col[~p.member & ~p.masked].abs().max() if (~p.member & ~p.masked).any() else 0.0) == 0.0
    assert float(col[p.masked].max() if p.masked.any() else 0.0) < 1e-40
    other = ref.out.clone()
    other[:form.N, 3] = 0
    assert float(other.abs().max()) == 0.0 and bool(p.member.any()) and (bool((~p.member).any()) or form.Nd <= 32)
    if family == "nbr2d":
        assert (ref.lse[0] - torch.log(p.n)).abs().max() < 1e-15


@pytest.mark.parametrize("family,case", [("local", (2, 20, 3, 64, 12, 11)), ("local", (1, 29, 1, 128, 15, 14)),
                                         ("win2d", (3, 8, 16, 1, 32, 4, 8, 2, 4)), ("win2d", (2, 6, 10, 1, 64, 3, 5, 2, 0)),
                                         ("nbr2d", (2, 4, 15, 2, 32, 7, 11)), ("nbr2d", (1, 16, 33, 1, 64, 3, 5))], ids=str)
def test_one_hot_groups_is_exact_in_float64(family, case):
    form = R.make_form(family, case)
    c = R.one_hot_groups(form, 77, BF)
    r, ref = R.reference(form, c.qkv, c.side, c.dout)
    D = form.h * form.hd
    N = form.N
    onehot = torch.zeros(form.B, form.h, form.Nd, form.Nd, dtype=F64)
    onehot[:, :, :N, :N].scatter_(-1, c.perm.unsqueeze(-1), 1.0)
    leak = float((r.P[:, :, :N] * (1 - onehot[:, :, :N])).max())
    print(f"{family} {case}: leak {leak:.1e}")
    assert leak < 1e-38
    assert (ref.out - c.O.double()).abs().max() < 1e-30 and (ref.dqkv[:, 2 * D:] - c.dV.double()).abs().max() < 1e-30
    assert float(ref.dqkv[:, :2 * D].abs().max()) < 1e-30
    assert torch.equal(c.qkv.float().to(BF), c.qkv) and float(c.O.abs().max()) <= 8


# ---- injected faults -----------------------------------------------------------------------------------------------------
def _verdict(k, name, bad, family, case, old_forward, build=None):
    """the fault `bad(c)` -> wrong tensor of output `name`, on the case's reference in both dtypes: the per-element gate must
    reject it; -> what the older aggregate gates say (bfloat16, float32)"""
    old = []
    for dtype in (BF, F32):
        c = R.case_reference(family, case, dtype) if build is None else build(dtype)
        want = c.ref[name]
        wrong = bad(c)
        assert R.worst_ratio(want, want, c.bound[name]) == 0.0
        ratio = R.worst_ratio(wrong, want, c.bound[name])
        verdict = R.old_forward_gate(wrong, want, dtype) if old_forward else R.old_backward_gate(wrong, want, dtype)
        print(f"fault {k} {dtype}: {int((wrong != want).sum())} elements, new gate ratio {ratio:.1f} (limit {R.limit(dtype)}), "
              f"old gate {'accepts' if verdict else 'rejects'}")
        assert ratio > R.limit(dtype), (k, dtype, ratio)
        old.append(verdict)
    assert tuple(old) == OLD_GATES[k], (k, old)


def test_fault_1_padding_key_masked():
    case = (1, 29, 1, 64, 15, 14)

    def bad(c):
        bias = R.dense_bias(c.form, c.side).clone()
        bias[:, :, c.form.N:] = R.NEG
        return R.reference(c.form, c.qkv, c.side, c.dout, bias=bias)[1].out
    _verdict(1, "out", bad, "local", case, True)


def test_fault_2_wrap_slot_reads_the_neighbouring_token():
    case = (2, 20, 3, 64, 12, 11)           # slot 0 reads token 0 - 11 + 20 = 9; the fault: 8

    def bad(c):
        B, N, h, hd, w, shift = case
        return R.reference(R.form_local(B, N, h, hd, w, shift, slot_token={0: N - shift - 1}), c.qkv, c.side, c.dout)[1].out
    _verdict(2, "out", bad, "local", case, True)


def test_fault_3_key_outside_the_clipped_box():
    case = (1, 5, 16, 1, 64, 3, 5)          # query (0, 0), 2 x 3 keys: column -1 staged as zeros and not masked

    def bad(c):
        out = c.ref["out"].clone()
        out[0, :64] /= 1.0 + math.exp(-float(c.ref["lse"][0, 0]))     # one more key of score 0 and value 0
        return out
    _verdict(3, "out", bad, "nbr2d", case, True)
    # the same fault in the corner of a 7 x 11 box (4 x 6 keys, so one more moves the row by 4 %): bfloat16 rounding of the row
    # is of that size (the model says so: ratio about 2), the older bfloat16 gate accepts it, the float32 gates do not
    for dtype in (BF, F32):
        c = R.case_reference("nbr2d", (2, 4, 15, 2, 32, 7, 11), dtype)
        out = c.ref["out"].clone()
        out[0, :32] /= 1.0 + math.exp(-float(c.ref["lse"][0, 0]))
        ratio = R.worst_ratio(out, c.ref["out"], c.bound["out"])
        print(f"7 x 11 corner, {dtype}: ratio {ratio:.1f}, old gate accepts: {R.old_forward_gate(out, c.ref['out'], dtype)}")
        assert dtype == BF or ratio > R.limit(dtype)
    assert R.old_forward_gate(out, c.ref["out"], F32) is False


def test_fault_4_additive_mask_as_minus_infinity():
    form = R.form_win2d(1, 1, 8, 1, 32, 1, 8, 0, 4)
    qkv, table = SR.pinned_mask_case()
    dout = torch.randn(8, 32, generator=torch.Generator().manual_seed(4))

    def build(dtype):
        q, g = qkv.to(dtype), dout.to(dtype)
        r, ref = R.reference(form, q, table, g)
        floor = R.float32_floor(form, q, table, g)
        return R.SimpleNamespace(form=form, qkv=q, side=table, dout=g, r=r, ref=vars(ref), bound=R.bounds(form, r, floor, dtype))

    def bad(c):
        return R.reference(form, c.qkv, c.side, c.dout, bias=R.dense_bias(form, c.side, mask_value=R.NEG))[1].out
    _verdict(4, "out", bad, "win2d", None, True, build=build)


def test_fault_5_corner_entry_of_the_table_gradient_dropped():
    case = (3, 8, 16, 1, 32, 4, 8, 2, 4)

    def bad(c):
        dt = c.ref["dtable"].clone()
        dt[c.form.TE - 1] = 0.0             # (wh - 1, ww - 1): query in the window's last slot, key in its first
        return dt
    _verdict(5, "dtable", bad, "win2d", case, False)
    # the same entry losing ONE window's pair: a few 1e-3 of the tensor's maximum
    for dtype in (BF, F32):
        c = R.case_reference("win2d", case, dtype)
        f = c.form
        tq, tk = int(torch.nonzero((f.win == 0) & (f.slot == f.n - 1))), int(torch.nonzero((f.win == 0) & (f.slot == 0)))
        assert int(f.idx[tq, tk]) == f.TE - 1
        dt = c.ref["dtable"].clone()
        dt[f.TE - 1, 0] -= c.r.dscore[0, 0, tq, tk]
        ratio = R.worst_ratio(dt, c.ref["dtable"], c.bound["dtable"])
        print(f"one pair of the corner entry, {dtype}: ratio {ratio:.1f}, old gate accepts: {R.old_backward_gate(dt, c.ref['dtable'], dtype)}")
        assert ratio > R.limit(dtype)


def test_fault_6_weight_zero_partner_counted_in_dv():
    case = (2, 6, 10, 1, 64, 3, 5, 2, 0)    # 15 tokens: row 14 is walked with itself as its partner, weight 0

    def bad(c):
        f = c.form
        D = f.h * f.hd
        toks = torch.nonzero(f.win == 0).flatten()
        tq = int(torch.nonzero((f.win == 0) & (f.slot == f.n - 1)))
        dqkv = c.ref["dqkv"].clone()
        dqkv[toks, 2 * D:2 * D + f.hd] += c.r.P[0, 0, tq, toks, None] * c.r.do[0, 0, tq][None, :]
        return dqkv
    _verdict(6, "dqkv", bad, "win2d", case, False)
