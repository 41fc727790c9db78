"""The window and neighbourhood attention kernels that keep their scores on the VALU (csrc/window_attn_impl.h: lgp.hip's
htrvt_attn_local_* / _local_shift_*, swin.hip's htrvt_attn_win2d_* with htrvt_rowsum_f32, svtr.hip's htrvt_attn_nbr2d_*)
through the C ABI, element by element, at the edges of their dispatch, in bfloat16 and float32.

Every expectation comes from tests/window_refs.py and is proved on the host by tests/test_window_refs_cpu.py: random cases
are held per element to C_GPU x the error model around the float64 reference (bfloat16) or to 8 x E32 x max|ref| (float32,
lse, the float32 sums), the structured cases (membership probe, one-hot, 1 x 1 windows and boxes) to exact values.  Every
output (out, dqkv, lse, dpad, dtable_partial, the reduced dtable) is cut out of a larger allocation, pre-filled with NaN (the
accumulated dtable with 0) and its guard bands in front and behind are compared afterwards.  The aggregate gates of
test_lgp_kernels_gpu.py, test_local_shift_gpu.py, test_swin_gpu.py and test_svtr_gpu.py stay where they are.

Worst |got - ref| / bound measured on an MI355X over the random cases of this file (gate: 2.0 bfloat16, 1.0 float32), next
to the host emulation's bfloat16 figure (window_refs.EMULATION_WORST):
                 bfloat16 (emulation)                                            float32
    1-D local    out 0.80 (0.80), dqkv 0.91 (0.91), dpad 0.91 (0.91)             out 0.17, dqkv 0.20, dpad 0.34
    2-D windows  out 0.84 (0.84), dqkv 0.95 (0.95), dtable 0.08 (0.13)           out 0.13, dqkv 0.19, dtable 0.26
    boxes        out 0.76 (0.76), dqkv 0.87 (0.87), lse 0.18 (0.15)              out 0.13, dqkv 0.30, lse 0.17
-- the kernels sit where the emulation sits: the model lacks no rounding point, and the float32 instances use a third of
their allowance at the most.  Membership probes: at most 0.49 ulp from 1 / n.  189 cases in 3.3 s.
Run against a library with three wrong-result mutations (a box key one column outside the map left unmasked, the -100 mask
of the 2-D forward as -inf, the 1-D wrap slot reading the token before its own) 102 of the cases fail: every shifted 1-D
case, every clipped box, the pinned mask."""
import pytest
import torch

import window_refs as R
from window_refs import BF, F32

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])


def _abi():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import lib
    from htrvt_amd.ops import dt, ptr, stream
    return lib, ptr, stream, dt


def _ok(rc):
    assert rc == 0, _abi()[0].htrvt_last_error().decode()


def _clean(outs):
    for name, t in outs.items():
        assert not torch.isnan(t.float()).any(), f"an element of {name} was not written"


def _gate(family, dtype, outs, c, names=None):
    """per element: |got - ref| <= limit x bound, for every output of the family"""
    for n in names or R.OUTPUTS[family]:
        ratio = R.worst_ratio(outs[n].detach().cpu(), c.ref[n], c.bound[n])
        print(f"RATIO {family} {'bf16' if dtype == BF else 'f32'} {n} {ratio:.3f}")
        assert ratio <= R.limit(dtype), (family, n, ratio)


def _dev(c, dtype):
    return c.qkv.to(dtype).cuda(), None if c.side is None else c.side.float().cuda(), None if c.dout is None else c.dout.to(dtype).cuda()


# ---- launches into guarded buffers ----------------------------------------------------------------------------------------
def local_fwd(case, qkv, bias, dtype):
    lib, ptr, stream, dt = _abi()
    B, N, h, hd, w, shift = case
    out = R.guarded((B * N, h * hd), dtype)
    if shift is None:
        _ok(lib.htrvt_attn_local_fwd(ptr(qkv), ptr(bias), ptr(out), B, N, h, hd, w, hd ** -0.5, dt(dtype), stream()))
    else:
        _ok(lib.htrvt_attn_local_shift_fwd(ptr(qkv), ptr(bias), ptr(out), B, N, h, hd, w, shift, hd ** -0.5, dt(dtype), stream()))
    return {"out": out}


def local_bwd(case, qkv, bias, dout, dtype, into=None):
    """into: the buffers of an earlier call, written again"""
    lib, ptr, stream, dt = _abi()
    B, N, h, hd, w, shift = case
    D = h * hd
    o = into or {"dqkv": R.guarded((B * N, 3 * D), dtype), "dpad": R.guarded((B, 2 * D), F32)}
    if shift is None:
        _ok(lib.htrvt_attn_local_bwd(ptr(qkv), ptr(bias), ptr(dout), ptr(o["dqkv"]), ptr(o["dpad"]), B, N, h, hd, w, hd ** -0.5,
                                     dt(dtype), stream()))
    else:
        _ok(lib.htrvt_attn_local_shift_bwd(ptr(qkv), ptr(bias), ptr(dout), ptr(o["dqkv"]), ptr(o["dpad"]), B, N, h, hd, w, shift,
                                           hd ** -0.5, dt(dtype), stream()))
    return o


def win2d_fwd(case, qkv, table, dtype):
    lib, ptr, stream, dt = _abi()
    B, H, W, h, hd, wh, ww, sh, sw = case
    out = R.guarded((B * H * W, h * hd), dtype)
    _ok(lib.htrvt_attn_win2d_fwd(ptr(qkv), ptr(table), ptr(out), B, H, W, h, hd, wh, ww, sh, sw, hd ** -0.5, dt(dtype), stream()))
    return {"out": out}


def win2d_bwd(case, qkv, table, dout, dtype):
    lib, ptr, stream, dt = _abi()
    B, H, W, h, hd, wh, ww, sh, sw = case
    D, TE = h * hd, (2 * wh - 1) * (2 * ww - 1)
    rows = lib.htrvt_attn_win2d_rows(B, H, W, h, wh, ww)
    assert rows == min(B * (H // wh) * (W // ww), 256)
    o = {"dqkv": R.guarded((B * H * W, 3 * D), dtype), "partial": R.guarded((rows, TE * h), F32),
         "dtable": R.guarded((TE, h), F32, fill=0.0)}                  # htrvt_rowsum_f32 adds to what dtable holds
    _ok(lib.htrvt_attn_win2d_bwd(ptr(qkv), ptr(table), ptr(dout), ptr(o["dqkv"]), ptr(o["partial"]), B, H, W, h, hd, wh, ww, sh, sw,
                                 hd ** -0.5, dt(dtype), stream()))
    _ok(lib.htrvt_rowsum_f32(ptr(o["partial"]), rows, TE * h, ptr(o["dtable"]), stream()))
    return o


def nbr2d_fwd(case, qkv, dtype):
    lib, ptr, stream, dt = _abi()
    B, H, W, h, hd, kh, kw = case
    o = {"out": R.guarded((B * H * W, h * hd), dtype), "lse": R.guarded((B * h, H * W), F32)}
    _ok(lib.htrvt_attn_nbr2d_fwd(ptr(qkv), ptr(o["out"]), ptr(o["lse"]), B, H, W, h, hd, kh, kw, hd ** -0.5, dt(dtype), stream()))
    return o


def nbr2d_bwd(case, qkv, fwd, dout, dtype):
    lib, ptr, stream, dt = _abi()
    B, H, W, h, hd, kh, kw = case
    o = {"dqkv": R.guarded((B * H * W, 3 * h * hd), dtype)}
    _ok(lib.htrvt_attn_nbr2d_bwd(ptr(qkv), ptr(fwd["out"]), ptr(dout), ptr(fwd["lse"]), ptr(o["dqkv"]), B, H, W, h, hd, kh, kw,
                                 hd ** -0.5, dt(dtype), stream()))
    return o


def run(family, case, qkv, side, dout, dtype):
    """forward and backward of one case -> {output: guarded device tensor}"""
    if family == "local":
        o = local_fwd(case, qkv, side, dtype)
        o.update(local_bwd(case, qkv, side, dout, dtype))
    elif family == "win2d":
        o = win2d_fwd(case, qkv, side, dtype)
        o.update(win2d_bwd(case, qkv, side, dout, dtype))
    else:
        o = nbr2d_fwd(case, qkv, dtype)
        o.update(nbr2d_bwd(case, qkv, o, dout, dtype))
    return o


# ---- random cases, per element -------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("case", R.LOCAL_FULL, ids=str)
def test_local_random_per_element(case, dtype):
    B, N, h, hd, w, shift = case
    lib, _, _, dt = _abi()
    assert (lib.htrvt_attn_local_supported(hd, w, dt(dtype)) if shift is None else
            lib.htrvt_attn_local_shift_supported(hd, w, shift, dt(dtype))) == 1
    c = R.case_reference("local", case, dtype)
    qkv, bias, dout = _dev(c, dtype)
    o = run("local", case, qkv, bias, dout, dtype)
    first = {n: o[n].clone() for n in ("dqkv", "dpad")}
    local_bwd(case, qkv, bias, dout, dtype, into=o)         # again into the same dqkv and dpad: written, not added to
    R.assert_guards_intact()
    _clean(o)
    _gate("local", dtype, o, c)
    assert torch.equal(o["dqkv"], first["dqkv"]) and torch.equal(o["dpad"], first["dpad"])
    if N % w == 0:                                          # no padding key
        assert float(o["dpad"].abs().max()) == 0.0
    else:
        assert float(o["dpad"].abs().min()) > 0.0           # every (image, head) slice of the k and v halves was written
    if w == 1:                                              # every token alone: out = v, dv = dO, dq = dk = 0, exactly
        D = h * hd
        assert torch.equal(o["out"], qkv[:, 2 * D:]) and torch.equal(o["dqkv"][:, 2 * D:], dout)
        assert float(o["dqkv"][:, :2 * D].float().abs().max()) == 0.0


@DTYPES
@pytest.mark.parametrize("case", R.WIN2D_CASES, ids=str)
def test_win2d_random_per_element(case, dtype):
    B, H, W, h, hd, wh, ww, sh, sw = case
    lib, _, _, dt = _abi()
    assert lib.htrvt_attn_win2d_supported(hd, wh, ww, dt(dtype)) == 1
    c = R.case_reference("win2d", case, dtype)
    qkv, table, dout = _dev(c, dtype)
    o = run("win2d", case, qkv, table, dout, dtype)
    R.assert_guards_intact()
    _clean(o)
    _gate("win2d", dtype, o, c)
    # the partial rows, added in float64
    rows = o["partial"].shape[0]
    summed = {"dtable": o["partial"].double().cpu().sum(0).reshape(c.form.TE, h)}
    _gate("win2d", dtype, summed, c, names=("dtable",))
    if (wh, ww) == (1, 1):                                  # every token alone
        D = h * hd
        assert torch.equal(o["out"], qkv[:, 2 * D:]) and torch.equal(o["dqkv"][:, 2 * D:], dout)
        assert float(o["dqkv"][:, :2 * D].float().abs().max()) == 0.0 and float(o["partial"].abs().max()) == 0.0
    print(f"items {c.form.items} rows {rows}")


@DTYPES
@pytest.mark.parametrize("case", R.NBR2D_CASES, ids=str)
def test_nbr2d_random_per_element(case, dtype):
    B, H, W, h, hd, kh, kw = case
    lib, _, _, dt = _abi()
    assert lib.htrvt_attn_nbr2d_supported(hd, kh, kw, dt(dtype)) == 1
    c = R.case_reference("nbr2d", case, dtype)
    qkv, _, dout = _dev(c, dtype)
    o = run("nbr2d", case, qkv, None, dout, dtype)
    R.assert_guards_intact()
    _clean(o)
    _gate("nbr2d", dtype, o, c)
    if (kh, kw) == (1, 1):
        # self only: out = v bit for bit and lse = scale q.k (gated above).  Not so the backward: it recomputes the score and
        # takes delta from dO . out, each summed in another order than the forward's score and dO . v, so P - 1 and dP - delta
        # are float32 residues (measured 4e-7 and 8e-7 of dq / dk), inside the gates above
        assert torch.equal(o["out"], qkv[:, 2 * h * hd:])


def test_nbr2d_tile_rows_by_the_workgroup_count():
    """TH = 8 only for bfloat16 hd 32 where 8-row tiles leave no more idle rows than 4-row tiles (H = 5, 8, 16 of the list).
    Read off the host's own count of workgroups, B heads ceil(H / TH) ceil(W / 16): a batch whose count reaches 2^31 with
    the other tile and stays below it with the expected one (or the other way round) is refused, or passed on to the null
    check, accordingly.  Nothing is launched: every buffer is null."""
    lib, _, stream, dt = _abi()
    for dtype in (BF, F32):
        for hd in (32, 64):
            for H in (1, 4, 5, 8, 9, 12, 16):
                th = R.nbr2d_tile_rows(hd, dtype, H)
                assert th == (8 if (dtype == BF and hd == 32 and H in (5, 8, 16)) else 4)
                other = 12 - th
                t_exp, t_other = -(-H // th), -(-H // other)
                rc = lib.htrvt_attn_nbr2d_fwd(None, None, None, 2 ** 30, H, 1, 2, hd, 7, 11, 0.1, dt(dtype), stream())
                assert rc != 0 and f"workgroups of {th} x 16" in lib.htrvt_last_error().decode(), (dtype, hd, H)
                if t_exp != t_other:
                    Bn = -(-2 ** 31 // max(t_exp, t_other))         # the larger count reaches 2^31, the smaller does not
                    assert Bn * min(t_exp, t_other) < 2 ** 31 <= Bn * max(t_exp, t_other)
                    rc = lib.htrvt_attn_nbr2d_fwd(None, None, None, Bn, H, 1, 1, hd, 7, 11, 0.1, dt(dtype), stream())
                    word = "workgroups" if t_exp > t_other else "null"
                    assert rc != 0 and word in lib.htrvt_last_error().decode(), (dtype, hd, H, lib.htrvt_last_error())


# ---- structured cases ----------------------------------------------------------------------------------------------------
# (family, case, probed token): a corner, a window or box border, for the 1-D kernels a slot beside the padding rows
PROBES = [("local", (1, 14, 1, 64, 15, 13), 0),("local", (2, 20, 3, 64, 12, 11), 8), ("local", (2, 20, 3, 128, 12, 11), 9),
          ("local", (1, 100, 1, 128, 12, None), 99), ("local", (1, 100, 1, 64, 12, None), 95),
          ("win2d", (1, 4, 8, 1, 32, 4, 8, 3, 7), 0), ("win2d", (3, 8, 16, 1, 32, 4, 8, 2, 4), 127),
          ("win2d", (2, 6, 10, 1, 64, 3, 5, 2, 0), 24), ("win2d", (1, 2, 32, 1, 128, 1, 32, 0, 31), 32),
          ("nbr2d", (2, 4, 15, 2, 32, 7, 11), 0), ("nbr2d", (1, 16, 17, 1, 32, 7, 11), 16 * 17 - 1),
          ("nbr2d", (1, 9, 33, 1, 32, 1, 11), 4 * 33 + 16), ("nbr2d", (1, 16, 33, 1, 64, 3, 5), 8 * 33 + 15)]


@DTYPES
@pytest.mark.parametrize("family,case,t0", PROBES, ids=str)
def test_membership_probe(family, case, t0, dtype):
    """window_refs.membership_probe: out[query] = 1 / n(query) within 2 ulp where the probed token is one of the query's keys,
    exactly 0 elsewhere (below 1e-40 across a -100 mask); lse of a box = log n"""
    form = R.make_form(family, case)
    image, head, channel = form.B - 1, form.h - 1, 5
    p = R.membership_probe(form, t0, channel, dtype, image=image, head=head)
    qkv = p.qkv.cuda()
    side = None if p.side is None else p.side.cuda()
    o = {"local": lambda: local_fwd(case, qkv, side, dtype), "win2d": lambda: win2d_fwd(case, qkv, side, dtype),
         "nbr2d": lambda: nbr2d_fwd(case, qkv, dtype)}[family]()
    R.assert_guards_intact()
    _clean(o)
    N = form.N
    out = o["out"].double().cpu().reshape(form.B, N, form.h, form.hd)
    col = out[image, :, head, channel]
    want = 1.0 / p.n
    err = ((col - want).abs() / R.ulp(want, dtype))[p.member]
    print(f"membership {family} {case}: {int(p.member.sum())} members, worst {float(err.max()):.2f} ulp")
    assert float(err.max()) <= 2.0
    rest = ~p.member & ~p.masked
    assert float(col[rest].abs().max() if rest.any() else 0.0) == 0.0
    assert float(col[p.masked].abs().max() if p.masked.any() else 0.0) < 1e-40
    out[image, :, head, channel] = 0.0
    assert float(out.abs().max()) == 0.0                    # no other image, head or channel sees the token
    if family == "nbr2d":
        lse = o["lse"].double().cpu()
        want = torch.log(p.n).expand(form.B * form.h, N)
        assert float(((lse - want).abs() / want.clamp_min(1.0)).max()) <= 4 * 2.0 ** -24    # logf and one product


@DTYPES
def test_pinned_additive_mask_per_element(dtype):
    """swin_refs.pinned_mask_case: the masked pairs score 181 before the -100, so they still carry nearly all the weight; a
    mask applied as -inf (or skipped) moves every row of the first region.  Forward and backward, per element.
    Four table entries are used only by pairs from the second region to the first, whose weight is exp(-100) / 4 = 9e-45:
    float64 keeps a gradient of 5e-43 there, float32 has no normal number below 1.2e-38 and the kernels' exp gives 0 -- the
    reason window_refs.bounds allows every element the smallest normal float32 (without it this case stood at 2.3 x its
    bound in exactly those entries)."""
    import swin_refs as SR
    case = (1, 1, 8, 1, 32, 1, 8, 0, 4)
    form = R.make_form("win2d", case)
    q, table = SR.pinned_mask_case()
    g = torch.randn(8, 32, generator=torch.Generator().manual_seed(4)).to(dtype)
    q = q.to(dtype)
    r, ref = R.reference(form, q, table, g)
    assert float(r.P[0, 0][form.differ].max()) > 0.1        # the masked pairs do carry weight
    c = R.SimpleNamespace(ref=vars(ref), bound=R.bounds(form, r, R.float32_floor(form, q, table, g), dtype), form=form)
    o = run("win2d", case, q.cuda(), table.float().cuda(), g.cuda(), dtype)
    R.assert_guards_intact()
    _clean(o)
    _gate("win2d", dtype, o, c)


ONE_HOT = [("local", (2, 20, 3, 64, 12, 11)), ("local", (1, 29, 1, 128, 15, 14)), ("local", (2, 17, 1, 64, 16, 15)),
           ("win2d", (3, 8, 16, 1, 32, 4, 8, 2, 4)), ("win2d", (2, 6, 10, 1, 64, 3, 5, 2, 0)), ("win2d", (1, 5, 10, 1, 128, 5, 5, 4, 4)),
           ("nbr2d", (2, 4, 15, 2, 32, 7, 11)), ("nbr2d", (1, 16, 33, 1, 64, 3, 5)), ("nbr2d", (1, 16, 17, 1, 32, 7, 11))]


@DTYPES
@pytest.mark.parametrize("family,case", ONE_HOT, ids=str)
def test_one_hot_is_exact(family, case, dtype):
    """window_refs.one_hot_groups: out and dv bit for bit, dq = dk = 0, no gradient for the padding rows or the table"""
    form = R.make_form(family, case)
    c = R.one_hot_groups(form, 300 + len(case) + form.N, dtype)
    qkv, side, dout = _dev(c, dtype)
    o = run(family, case, qkv, side, dout, dtype)
    R.assert_guards_intact()
    _clean(o)
    D = form.h * form.hd
    assert torch.equal(o["out"].float().cpu(), c.O)
    assert torch.equal(o["dqkv"][:, 2 * D:].float().cpu(), c.dV)
    assert float(o["dqkv"][:, :2 * D].float().abs().max()) == 0.0
    if family == "local":
        assert float(o["dpad"].abs().max()) == 0.0
    if family == "win2d":
        assert float(o["partial"].abs().max()) == 0.0 and float(o["dtable"].abs().max()) == 0.0


@DTYPES
@pytest.mark.parametrize("family,case", [("local", (2, 20, 3, 128, 12, 11)), ("win2d", (3, 8, 16, 1, 32, 4, 8, 2, 4)),
                                         ("nbr2d", (2, 4, 15, 2, 32, 7, 11))], ids=str)
def test_two_launches_give_the_same_bits(family, case, dtype):
    c = R.case_reference(family, case, dtype)
    qkv, side, dout = _dev(c, dtype)
    a, b = run(family, case, qkv, side, dout, dtype), run(family, case, qkv, side, dout, dtype)
    R.assert_guards_intact()
    for n in a:
        assert torch.equal(a[n], b[n]), n
