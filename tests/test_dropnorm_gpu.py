"""csrc/dropnorm.hip through the C ABI, per element: htrvt_drop_add_ln_fwd and htrvt_layernorm_bwd_drop against the float64
restatements of tests/conformer_dropout_refs.py and the numpy restatement of the masks (attn_dropout_refs.keep_elems).

Shapes: rows 1 / 5 / 9 / 4101 with rows_per_sample = 3 (a sample boundary inside a workgroup's four rows; 4101 rows are past
the backward's 1024-block grid, so its waves loop), D filling every chunks-per-lane instance (1 ... 4 16-byte chunks per lane)
fully and partly, rates (p, p_path) none / elements only / samples only / both.
Exact: on x = 1, res = 0 the stored s is 0 or ONE other value, and the mask read off it equals the host mask element for
element; dxb is 0 exactly where the mask drops; ds and partial equal htrvt_layernorm_bwd's bit for bit; NULL statistics
outputs change nothing; canary rows behind every output survive; refused calls write nothing.
Otherwise per element against float64 over the same (already rounded) inputs, relative to the reference's largest magnitude:
gate = 8 * E32 (+ 2^-8 |ref| for a bfloat16 output), E32 = kernel_refs.e32, the float32 evaluation error of the reference
itself on these inputs -- nothing in a gate comes from the kernel under test.  y, mean and rstd are compared with the
float64 LayerNorm of the s the kernel STORED, after s has passed its own check (so a last-bit difference in s is not counted
twice); the backward takes that s and the reference's statistics (rounded to float32) as inputs.
With one row a statistic is ONE number and its E32 one draw between 0 and 2^-24; the inputs of a case are redrawn while that
draw is below 2^-26 (a gate under the spacing of the float32 the kernel stores); the rule reads the reference alone.
Every comparison prints E32, gate and observed error (`pytest -s`).  Measured on an MI355X, worst over all parametrised
cases of an output (errors relative to max |ref|; a bfloat16 gate is 2^-8 = 3.9e-3 plus 8 * E32):

  output              E32 (range)        worst observed     worst observed / gate
  s      bf16 / f32   0 .. 1.1e-7        3.8e-3 / 1.1e-7    0.97 / 0.13
  y      bf16 / f32   1.6e-8 .. 6.8e-7   3.5e-3 / 6.8e-7    0.90 / 0.47
  mean, rstd          0 .. 1.7e-7        1.7e-7 / 1.9e-7    0.34 / 0.47   (before the redraw rule one one-row case, float32
                                                            D = 264 without rates, drew E32(rstd) = 2.6e-9: observed 6.2e-8,
                                                            one float32 ulp, against a gate of 2.1e-8)
  ds     bf16 / f32   1.3e-8 .. 1.4e-7   3.6e-3 / 1.3e-7    0.91 / 0.17
  dxb    bf16 / f32   1.3e-8 .. 1.8e-7   3.6e-3 / 1.6e-7    0.93 / 0.22
  dgamma / dbeta      0 .. 3.7e-7        3.6e-7 / 3.2e-7    0.35 / 0.4
  fused against the two launches: s, y, mean, rstd, ds, dgamma, dbeta bit-equal in both dtypes
"""
import numpy as np
import pytest
import torch

import attn_dropout_refs as A
import conformer_dropout_refs as DR
import kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
EPS = float(torch.tensor(1e-6, dtype=F32))
RPS = 3
SEEDS = (0x1234567ABCDEF, 0x0FEDCBA987654)
WIDTHS = {BF: [8, 264, 768, 2048], F32: [4, 264, 768, 1024]}
RATES = [(0.0, 0.0), (0.1, 0.0), (0.0, 0.4), (0.5, 0.4)]


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import colsum, dt, ptr, stream
    return lib, check, ptr, stream, dt, colsum


def _check(name, got, ref, err, bf16_out):
    ok, obs = R.gate_check(name, got.detach().cpu(), ref, err, bf16_out)
    assert ok, f"{name}: observed {obs:.3e} of max|ref| is outside 8 * E32 = {8 * err:.3e}" + (" + one bf16 ulp" if bf16_out else "")


def _canary(*shape, dtype=F32):
    """a buffer of one more row than `shape`, filled with 7: the last row must survive"""
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), 7.0, dtype=dtype, device="cuda")


def _intact(*bufs):
    for b in bufs:
        assert (b[-1] == 7).all()


@pytest.mark.parametrize("p,p_path", RATES)
@pytest.mark.parametrize("rows", [1, 5, 9, 4101])
@pytest.mark.parametrize("dtype,D", [(d, D) for d in (BF, F32) for D in WIDTHS[d]])
def test_drop_add_ln_forward_and_backward(dtype, D, rows, p, p_path):
    lib, check, ptr, stream, dt, colsum = _lib()
    bf, dti = dtype == BF, dt(dtype)
    with_res = not (p == 0.0 and p_path > 0)                     # one of the rate pairs runs the backward without dres
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device="cuda") if p > 0 or p_path > 0 else None
    keepE, keepS = DR.site_masks(SEEDS, rows, D, RPS, p, p_path)
    keep = torch.from_numpy(keepE & np.repeat(keepS, RPS)[:rows, None])
    factor = DR.site_factor(SEEDS, rows, D, RPS, p, p_path)
    print(f"\ndropnorm {dtype} D={D} rows={rows} p={p} p_path={p_path}: kept {float(keep.double().mean()):.3f}")

    def fwd(x_, res_, s, y, mean, rstd):
        check(lib.htrvt_drop_add_ln_fwd(ptr(x_), ptr(res_), ptr(seeds), p, p_path, RPS, ptr(gamma_d), ptr(beta_d), ptr(s), ptr(y),
                                        ptr(mean), ptr(rstd), rows, D, EPS, dti, stream()), "drop_add_ln_fwd")

    # ---- the mask, exactly: x = 1, res = 0
    gamma_d = beta_d = torch.ones(D, device="cuda")
    s1, y1 = _canary(rows, D, dtype=dtype), _canary(rows, D, dtype=dtype)
    ones = torch.ones(rows, D, dtype=dtype, device="cuda")
    fwd(ones, torch.zeros_like(ones), s1, y1, None, None)
    got = s1[:rows].float().cpu()
    assert torch.equal(got != 0, keep)
    scale = np.float32(A.scale_of(p)) * np.float32(A.scale_of(p_path))
    kept_values = got[keep].unique()
    assert kept_values.numel() <= 1
    if kept_values.numel():
        assert float(kept_values[0]) == float(torch.tensor(float(scale)).to(dtype))
    _intact(s1, y1)

    # ---- forward.  The inputs are redrawn while the reference's OWN float32 evaluation of a statistic lands within a quarter
    # of a float32 ulp (2^-26) of its float64 value: with one row a statistic is one number, its E32 one draw between 0 and
    # 2^-24, and 8 times a lucky draw is a gate below the spacing of the float32 the kernel has to store (seen: E32 2.6e-9).
    # The rule looks at the reference alone, never at the kernel's mean or rstd.
    for draw in range(8):
        g = torch.Generator().manual_seed(rows * 7 + D + 1000 * draw)
        x, res = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(dtype), torch.randn(rows, D, generator=g).to(dtype)
        gamma, beta = torch.randn(D, generator=g) + 1, torch.randn(D, generator=g)
        dy, dres = torch.randn(rows, D, generator=g).to(dtype), torch.randn(rows, D, generator=g).to(dtype)
        x_d, res_d, gamma_d, beta_d = x.cuda(), res.cuda(), gamma.cuda(), beta.cuda()
        s, y, mean, rstd = _canary(rows, D, dtype=dtype), _canary(rows, D, dtype=dtype), _canary(rows), _canary(rows)
        fwd(x_d, res_d, s, y, mean, rstd)
        (s_r,), (es,) = R.e32(DR.drop_add, [x.float(), res.float(), factor])
        _check("s", s[:rows].float(), s_r, es, bf)
        sk = s[:rows].float().cpu()                              # as stored: what y and the statistics are taken from
        (y_r, mean_r, rstd_r), (ey, em, er) = R.e32(lambda a, b, c: DR.drop_add_ln_fwd(a, b, c, EPS), [sk, gamma, beta])
        if not any(0 < e < 2.0 ** -26 for e in (em, er)):
            break
        print(f"  redraw: E32 of mean / rstd {em:.1e} / {er:.1e}")
    else:
        raise AssertionError("no draw with a typical E32")
    _check("y", y[:rows].float(), y_r, ey, bf)
    _check("mean", mean[:rows], mean_r, em, False)
    _check("rstd", rstd[:rows], rstd_r, er, False)
    _intact(s, y, mean, rstd)
    s2, y2 = torch.empty_like(s), torch.empty_like(y)
    fwd(x_d, res_d, s2, y2, None, None)
    assert torch.equal(s2[:rows], s[:rows]) and torch.equal(y2[:rows], y[:rows])

    # ---- backward at the stored s, the statistics the reference's
    mean_i, rstd_i = mean_r.float(), rstd_r.float()
    nblk = lib.htrvt_layernorm_bwd_blocks(rows)
    dy_d, dres_d, mean_d, rstd_d = dy.cuda(), (dres.cuda() if with_res else None), mean_i.cuda(), rstd_i.cuda()
    s_in = s[:rows].contiguous()
    ds, dxb, partial = _canary(rows, D, dtype=dtype), _canary(rows, D, dtype=dtype), _canary(nblk, 2, D)
    check(lib.htrvt_layernorm_bwd_drop(ptr(dy_d), ptr(s_in), ptr(mean_d), ptr(rstd_d), ptr(gamma_d), ptr(dres_d), ptr(seeds), p,
                                       p_path, RPS, ptr(ds), ptr(dxb), ptr(partial), rows, D, dti, stream()), "layernorm_bwd_drop")

    def ref(dy_, s_, m_, r_, ga_, dres_, f_):
        return DR.layernorm_bwd_drop(dy_, s_, m_, r_, ga_, dres_ if with_res else None, f_)
    (ds_r, dxb_r, dg_r, db_r), (eds, edxb, edg, edb) = R.e32(ref, [dy.float(), sk, mean_i, rstd_i, gamma, dres.float(), factor])
    _check("ds", ds[:rows].float(), ds_r, eds, bf)
    _check("dxb", dxb[:rows].float(), dxb_r, edxb, bf)
    assert bool((dxb[:rows].cpu()[~keep] == 0).all())
    dgb = torch.zeros(2 * D, device="cuda")
    colsum(partial, nblk, 2 * D, 2 * D, dgb, dti=0)
    _check("dgamma", dgb[:D], dg_r, edg, False)
    _check("dbeta", dgb[D:], db_r, edb, False)
    _intact(ds, dxb, partial)
    # ds and partial are htrvt_layernorm_bwd's
    ds0, partial0 = torch.empty(rows, D, dtype=dtype, device="cuda"), torch.empty(nblk, 2, D, device="cuda")
    check(lib.htrvt_layernorm_bwd(ptr(dy_d), ptr(s_in), ptr(mean_d), ptr(rstd_d), ptr(gamma_d), ptr(dres_d), ptr(ds0), ptr(partial0),
                                  rows, D, dti, stream()), "layernorm_bwd")
    assert torch.equal(ds0, ds[:rows]) and torch.equal(partial0, partial[:nblk])


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_the_two_launch_route_draws_the_same_mask(dtype):
    """htrvt_residual_dropout + htrvt_layernorm_fwd from the same seeds: the same mask (s equals res at the same elements),
    values within a last bit; the backward's ds and parameter gradients bit for bit, dxb with the same zeros"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    rows, D, p, pp = 37, 264, 0.5, 0.4
    g = torch.Generator().manual_seed(5)
    x, res, dy = [torch.randn(rows, D, generator=g).to(dtype).cuda() for _ in range(3)]
    gamma, beta = (torch.randn(D, generator=g) + 1).cuda(), torch.randn(D, generator=g).cuda()
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device="cuda")
    s, y, mean, rstd = seq_ops.drop_add_ln_fwd(x, res, RPS, seeds, p, pp, gamma, beta, EPS)
    s2 = seq_ops.residual_dropout(x, res, RPS, seeds, p, pp)
    y2, mean2, rstd2 = seq_ops.layernorm_fwd(s2, gamma, beta, EPS)
    tol = 2.0 ** -7 if dtype == BF else 2.0 ** -22
    assert torch.equal(s == res, s2 == res) and 0.2 < float((s == res).double().mean()) < 0.95
    assert bool(((s.double() - s2.double()).abs() <= tol * s2.double().abs()).all())
    print(f"\n{dtype}: s bit-equal {torch.equal(s, s2)}, y bit-equal {torch.equal(y, y2)}")
    if torch.equal(s, s2):
        assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    ds, dxb = seq_ops.layernorm_bwd_drop(dy, s, mean, rstd, gamma, dg, db, RPS, seeds, p, pp)
    dg2, db2 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    ds2 = seq_ops.layernorm_bwd(dy, s, mean, rstd, gamma, dg2, db2)
    dxb2 = seq_ops.residual_dropout(ds2, None, RPS, seeds, p, pp)
    assert torch.equal(ds, ds2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    assert torch.equal(dxb == 0, dxb2 == 0)
    # the branch's gradient is formed from the unrounded ds: within one rounding of the two-launch route's
    assert bool(((dxb.double() - dxb2.double()).abs() <= tol * dxb2.double().abs()).all())


def test_refusals_launch_nothing():
    lib, check, ptr, stream, dt, _ = _lib()
    rows = 5
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device="cuda")
    for dtype, bad_d, wide_d, ok_d in ((BF, 12, 2056, 16), (F32, 6, 1028, 16)):
        dti, off = dt(dtype), (4 if dtype == F32 else 2)
        D = wide_d
        x = torch.ones(rows + 1, D, dtype=dtype, device="cuda")
        out = [torch.full((rows + 1, D), 7.0, dtype=dtype, device="cuda") for _ in range(2)]
        vec, st_, partial = torch.ones(D, device="cuda"), torch.ones(rows, device="cuda"), torch.full((2, 2, D), 7.0, device="cuda")

        def both(d_, p, pp, sd, rps=RPS, x_p=ptr(x), o_p=ptr(out[0])):
            return (lib.htrvt_drop_add_ln_fwd(x_p, x_p, sd, p, pp, rps, ptr(vec), ptr(vec), o_p, ptr(out[1]), ptr(st_), ptr(st_), rows,
                                              d_, EPS, dti, stream()),
                    lib.htrvt_layernorm_bwd_drop(x_p, x_p, ptr(st_), ptr(st_), ptr(vec), None, sd, p, pp, rps, o_p, ptr(out[1]),
                                                 ptr(partial), rows, d_, dti, stream()))
        bad = {"D off the vector": both(bad_d, 0.1, 0.0, ptr(seeds)), "D too wide": both(wide_d, 0.1, 0.0, ptr(seeds)),
               "p = 1": both(ok_d, 1.0, 0.0, ptr(seeds)), "p < 0": both(ok_d, -0.1, 0.0, ptr(seeds)),
               "p_path = 1": both(ok_d, 0.0, 1.0, ptr(seeds)), "no seeds, p > 0": both(ok_d, 0.1, 0.0, None),
               "no seeds, p_path > 0": both(ok_d, 0.0, 0.4, None), "rows_per_sample = 0": both(ok_d, 0.1, 0.0, ptr(seeds), rps=0),
               "input unaligned": both(ok_d, 0.1, 0.0, ptr(seeds), x_p=ptr(x) + off),
               "output unaligned": both(ok_d, 0.1, 0.0, ptr(seeds), o_p=ptr(out[0]) + off),
               "missing output": both(ok_d, 0.1, 0.0, ptr(seeds), o_p=None),
               "dtype": (lib.htrvt_drop_add_ln_fwd(ptr(x), ptr(x), ptr(seeds), 0.1, 0.0, RPS, ptr(vec), ptr(vec), ptr(out[0]), ptr(out[1]),
                                                   None, None, rows, ok_d, EPS, 2, stream()),)}
        for what, rcs in bad.items():
            assert all(rc != 0 for rc in rcs), (what, rcs)
        assert lib.htrvt_last_error()
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in out) and bool((partial == 7).all())
