"""LayerNorm, softmax, sequence-whiten and every BatchNorm piece through the C ABI against tests/kernel_refs.py.

Exact (torch.equal) wherever the inputs make every intermediate representable: bn_apply*, bn_bwd_apply*, bn_bwd_reduce,
the parameter-gradient accumulation of bn_bwd_finalize, the refused shapes, the STREAM-size launches.  Otherwise per
element against the float64 reference over the same (already rounded) inputs, relative to the reference's largest
magnitude: gate = 8 * E32 (+ 2^-8 |ref| for a bfloat16 output), E32 = the float32 evaluation error of the reference
itself on these inputs (kernel_refs.e32) -- nothing in a gate comes from the kernel under test.

Every non-exact comparison prints its E32, gate and observed error (`pytest -s`).  Measured on an MI355X, over all
parametrised cases of an output (errors relative to max |ref|; a bfloat16 gate is 2^-8 = 3.9e-3 plus 8 * E32):

  output                       E32 (range)        worst observed   worst observed / gate
  layernorm fwd y     bf16     2.7e-8 .. 1.3e-5   3.1e-3           0.80
  layernorm fwd y     f32      9.5e-6 .. 4.7e-4   4.7e-4           0.13    (rows with mean 100, sigma 0.1)
  layernorm fwd mean / rstd    0 .. 2.2e-7        1.7e-7 / 3.1e-7  0.14 / 0.45
  layernorm bwd dx    bf16     3.3e-8 .. 1.8e-7   3.4e-3           0.86
  layernorm bwd dx    f32      3.7e-8 .. 1.7e-7   1.1e-7           0.19
  layernorm bwd dgamma / dbeta 9.1e-9 .. 2.4e-7   2.0e-7 / 1.9e-7  0.22 / 0.23
  softmax             bf16     0 .. 6.4e-7        2.2e-3           0.57
  softmax             f32      0 .. 6.4e-7        6.4e-7           0.14
  softmax bwd         bf16/f32 4.9e-8 .. 1.5e-7   3.2e-3 / 9.9e-8  0.82 / 0.18
  seq_whiten y / stats         2.6e-8 .. 1.7e-7   1.8e-7 / 5.9e-8  0.13
  seq_whiten bwd      bf16/f32 6.1e-8 .. 1.2e-7   2.9e-3 / 1.2e-7  0.74
  bn_finalize (6 outputs)      0 .. 1.6e-7        1.2e-7           0.46    (shift)
  bn_eval_coeffs               2.9e-8 .. 1.3e-7   8.2e-8           0.13
  bn backward dx      bf16     6.3e-8 .. 1.2e-7   3.1e-3           0.79
  bn backward dx      f32      6.5e-8 .. 1.3e-7   7.9e-8           0.13
  bn backward dgamma / dbeta   2.4e-8 .. 3.9e-7   3.2e-7 / 2.0e-7  0.46 / 0.28
  bn backward coef [3][C]      1.9e-8 .. 7.0e-8   1.3e-7           0.71
"""
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
EPS_LN = float(torch.tensor(1e-6, dtype=F32))        # the value the float argument of the entry points carries
EPS_BN = float(torch.tensor(1e-5, dtype=F32))
SET = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)              # exactly representable coefficients of the exact tests


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import colsum, dt, ptr, stream
    return lib, check, ptr, stream, dt, colsum


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pick(g, n, values=SET):
    return torch.tensor(values)[torch.randint(0, len(values), (n,), generator=g)]


def _check(name, got, ref, err, bf16_out):
    ok, obs = R.gate_check(name, got.detach().cpu(), ref, err, bf16_out)
    assert ok, f"{name}: observed {obs:.3e} of max|ref| is outside 8 * E32 = {8 * err:.3e}" + (" + one bf16 ulp" if bf16_out else "")


# ====================================================================== LayerNorm
LN_D = {BF: [8, 64, 512, 768, 1032, 2048], F32: [4, 64, 256, 768, 1000, 1024]}


@pytest.mark.parametrize("rows", [1, 3, 37, 4100])
@pytest.mark.parametrize("dtype,D", [(d, D) for d in (BF, F32) for D in LN_D[d]])
def test_layernorm_forward_and_backward(dtype, D, rows):
    """every NK instance of the backward full and partly filled (chunks per lane 1..4), rows above 4 * 1024 (waves loop),
    rows with mean >> spread, NULL statistics outputs, dres NULL / given, dgamma / dbeta accumulated through colsum"""
    lib, check, ptr, stream, dt, colsum = _lib()
    g = _gen(rows * 7 + D)
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    x[::3] = torch.randn((rows + 2) // 3, D, generator=g) * 0.1 + 100.0
    x = x.to(dtype)
    gamma, beta = torch.randn(D, generator=g) + 1, torch.randn(D, generator=g)
    dy, dres = torch.randn(rows, D, generator=g).to(dtype), torch.randn(rows, D, generator=g).to(dtype)
    bf = dtype == BF
    print(f"\nlayernorm {dtype} D={D} rows={rows}")
    (y_r, mean_r, rstd_r), (ey, em, er) = R.e32(lambda a, b, c: R.layernorm_fwd(a, b, c, EPS_LN), [x.float(), gamma, beta])

    x_d, gamma_d, beta_d = x.cuda(), gamma.cuda(), beta.cuda()
    y = torch.full((rows + 1, D), 7.0, dtype=dtype, device="cuda")
    mean, rstd = torch.full((rows + 1,), 7.0, device="cuda"), torch.full((rows + 1,), 7.0, device="cuda")
    check(lib.htrvt_layernorm_fwd(ptr(x_d), ptr(gamma_d), ptr(beta_d), ptr(y), ptr(mean), ptr(rstd), rows, D, EPS_LN, dt(dtype),
                                  stream()), "layernorm_fwd")
    _check("fwd y", y[:rows].float(), y_r, ey, bf)
    _check("fwd mean", mean[:rows], mean_r, em, False)
    _check("fwd rstd", rstd[:rows], rstd_r, er, False)
    assert (y[rows] == 7).all() and mean[rows] == 7 and rstd[rows] == 7
    y2 = torch.empty(rows, D, dtype=dtype, device="cuda")
    check(lib.htrvt_layernorm_fwd(ptr(x_d), ptr(gamma_d), ptr(beta_d), ptr(y2), None, None, rows, D, EPS_LN, dt(dtype), stream()),
          "layernorm_fwd without statistics")
    assert torch.equal(y2, y[:rows])

    # backward: the statistics are INPUTS (the reference's, rounded to float32)
    mean_i, rstd_i = mean_r.float(), rstd_r.float()
    dg0, db0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    nblk = lib.htrvt_layernorm_bwd_blocks(rows)
    assert nblk == min((rows + 3) // 4, 1024)
    dy_d, dres_d, mean_d, rstd_d = dy.cuda(), dres.cuda(), mean_i.cuda(), rstd_i.cuda()
    for with_res in (False, True):
        def ref(dy_, x_, m_, r_, ga_, dres_, dg0_, db0_):
            dx_, dga_, dbe_ = R.layernorm_bwd(dy_, x_, m_, r_, ga_, dres_ if with_res else None)
            return dx_, dga_ + dg0_, dbe_ + db0_
        (dx_r, dg_r, db_r), (edx, edg, edb) = R.e32(ref, [dy.float(), x.float(), mean_i, rstd_i, gamma, dres.float(), dg0, db0])
        dx = torch.full((rows + 1, D), 7.0, dtype=dtype, device="cuda")
        partial = torch.full((nblk + 1, 2, D), 7.0, device="cuda")
        check(lib.htrvt_layernorm_bwd(ptr(dy_d), ptr(x_d), ptr(mean_d), ptr(rstd_d), ptr(gamma_d), ptr(dres_d) if with_res else None,
                                      ptr(dx), ptr(partial), rows, D, dt(dtype), stream()), "layernorm_bwd")
        dgb = torch.cat([dg0, db0]).cuda()          # weight and bias gradients adjacent: one column sum, as Engine.ln_bwd
        colsum(partial, nblk, 2 * D, 2 * D, dgb, dti=0)
        _check(f"bwd dx (dres {with_res})", dx[:rows].float(), dx_r, edx, bf)
        _check("bwd dgamma", dgb[:D], dg_r, edg, False)
        _check("bwd dbeta", dgb[D:], db_r, edb, False)
        assert (dx[rows] == 7).all() and (partial[nblk] == 7).all()


@pytest.mark.parametrize("dtype,D", [(BF, 2056), (BF, 12), (F32, 1028), (F32, 6)])
def test_layernorm_refuses_unsupported_widths_without_launching(dtype, D):
    lib, check, ptr, stream, dt, _ = _lib()
    rows = 5
    x = torch.ones(rows, D, dtype=dtype, device="cuda")
    vec = torch.ones(D, device="cuda")
    st = torch.ones(rows, device="cuda")
    out = torch.full((rows, D), 7.0, dtype=dtype, device="cuda")
    partial = torch.full((2, 2, D), 7.0, device="cuda")
    assert lib.htrvt_layernorm_fwd(ptr(x), ptr(vec), ptr(vec), ptr(out), None, None, rows, D, EPS_LN, dt(dtype), stream()) != 0
    assert lib.htrvt_layernorm_bwd(ptr(x), ptr(x), ptr(st), ptr(st), ptr(vec), None, ptr(out), ptr(partial), rows, D, dt(dtype),
                                   stream()) != 0
    assert lib.htrvt_last_error()
    torch.cuda.synchronize()
    assert (out == 7).all() and (partial == 7).all()


# ====================================================================== softmax
def _softmax_inputs(g, rows, n, brows):
    s = torch.randn(rows, n, generator=g)
    s[::2] = (torch.rand((rows + 1) // 2, n, generator=g) - 0.5) * 80.0          # scores spread over +-40
    bias = torch.randn(brows, n, generator=g)
    for r in range(brows):                                                        # the variants' window mask: -1e30 outside
        lo = (r * 3) % n
        keep = torch.zeros(n, dtype=torch.bool)
        keep[lo:lo + max(n // 4, 1)] = True
        bias[r, ~keep] = -1e30
    bias[brows - 1] = -1e30                                                       # a row masked everywhere
    return s, bias


@pytest.mark.parametrize("n", [4, 128, 132, 256, 1024])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_softmax_rows_and_backward(dtype, n):
    lib, check, ptr, stream, dt, _ = _lib()
    rows, brows = 37, 5                    # rows not a multiple of 4 (waves per block) nor of bias_rows
    g = _gen(n)
    s, bias = _softmax_inputs(g, rows, n, brows)
    bf = dtype == BF
    print(f"\nsoftmax {dtype} n={n}")
    s_d, bias_d = s.cuda(), bias.cuda()
    for b, b_d, name in ((None, None, "plain"), (bias, bias_d, "bias")):
        (p_r,), (ep,) = R.e32(lambda a, c=None: R.softmax_rows(a, c), [s] + ([b] if b is not None else []))
        p = torch.full((rows + 1, n), 7.0, dtype=dtype, device="cuda")
        check(lib.htrvt_softmax_rows(ptr(s_d), ptr(p), rows, n, dt(dtype), ptr(b_d), brows if b is not None else 0, stream()),
              "softmax_rows")
        assert torch.isfinite(p).all() and (p[rows] == 7).all()
        _check(f"softmax {name}", p[:rows].float(), p_r, ep, bf)
        if b is not None:
            masked = (bias[torch.arange(rows) % brows] == -1e30)
            full = masked.all(1)
            assert full.any() and (p[:rows].float().cpu()[masked & ~full[:, None]] == 0).all()
    # backward over the (rounded) reference probabilities
    p_i = R.softmax_rows(s.double(), None).to(dtype)
    dp = torch.randn(rows, n, generator=g)
    scale = 0.125
    (ds_r,), (eds,) = R.e32(lambda a, c: R.softmax_bwd_rows(a, c, scale), [p_i.float(), dp])
    p_d, dp_d = p_i.cuda(), dp.cuda()
    ds = torch.full((rows + 1, n), 7.0, dtype=dtype, device="cuda")
    check(lib.htrvt_softmax_bwd_rows(ptr(p_d), ptr(dp_d), ptr(ds), rows, n, scale, dt(dtype), stream()), "softmax_bwd_rows")
    _check("softmax bwd", ds[:rows].float(), ds_r, eds, bf)
    assert (ds[rows] == 7).all()


@pytest.mark.parametrize("n", [1028, 6])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_softmax_refuses_unsupported_widths_without_launching(dtype, n):
    lib, check, ptr, stream, dt, _ = _lib()
    rows = 3
    s = torch.zeros(rows, n, device="cuda")
    pin = torch.zeros(rows, n, dtype=dtype, device="cuda")
    out = torch.full((rows, n), 7.0, dtype=dtype, device="cuda")
    assert lib.htrvt_softmax_rows(ptr(s), ptr(out), rows, n, dt(dtype), None, 0, stream()) != 0
    assert lib.htrvt_softmax_bwd_rows(ptr(pin), ptr(s), ptr(out), rows, n, 1.0, dt(dtype), stream()) != 0
    torch.cuda.synchronize()
    assert (out == 7).all()
    n_ok = 8
    assert lib.htrvt_softmax_rows(ptr(s), ptr(out), rows, n_ok, dt(dtype), ptr(s), 0, stream()) != 0      # a bias needs bias_rows > 0
    torch.cuda.synchronize()
    assert (out == 7).all()


# ====================================================================== sequence whiten
@pytest.mark.parametrize("N,C", [(5, 9), (37, 80), (128, 80), (1, 3)])
def test_seq_whiten_forward_and_backward(N, C):
    """N*C below 256, not a multiple of 256 and a multiple of it; the backward with ldo = C and ldo > C (pad columns
    pre-filled with NaN must stay NaN) in both output types; stats NULL in the forward"""
    lib, check, ptr, stream, dt, _ = _lib()
    B, NC = 3, N * C
    g = _gen(NC)
    x = torch.randn(B, NC, generator=g) * 3 + 5
    print(f"\nseq_whiten N={N} C={C}")
    (y_r, st_r), (ey, es) = R.e32(lambda a: R.seq_whiten_fwd(a, EPS_BN), [x])
    x_d = x.cuda()
    y = torch.full((B + 1, NC), 7.0, device="cuda")
    stats = torch.full((B + 1, 2), 7.0, device="cuda")
    check(lib.htrvt_seq_whiten_fwd(ptr(x_d), ptr(y), ptr(stats), B, NC, EPS_BN, 0, stream()), "seq_whiten_fwd")
    _check("whiten y", y[:B], y_r, ey, False)
    _check("whiten stats", stats[:B], st_r, es, False)
    assert (y[B] == 7).all() and (stats[B] == 7).all()
    y2 = torch.empty(B, NC, device="cuda")
    check(lib.htrvt_seq_whiten_fwd(ptr(x_d), ptr(y2), None, B, NC, EPS_BN, 0, stream()), "seq_whiten_fwd without stats")
    assert torch.equal(y2, y[:B])
    assert lib.htrvt_seq_whiten_fwd(ptr(x_d), ptr(y2), None, B, NC, EPS_BN, 1, stream()) != 0          # logits are float32

    y_i, st_i = y_r.float(), st_r.float()
    dy = torch.randn(B, NC, generator=g)
    (dx_r,), (edx,) = R.e32(R.seq_whiten_bwd, [dy, y_i, st_i])
    dy_d, y_d, st_d = dy.cuda(), y_i.cuda(), st_i.cuda()
    for dtype in (BF, F32):
        for ldo in (C, C + 8):
            dx = torch.full((B * N + 1, ldo), float("nan"), dtype=dtype, device="cuda")
            check(lib.htrvt_seq_whiten_bwd(ptr(dy_d), ptr(y_d), ptr(st_d), ptr(dx), B, N, C, ldo, dt(dtype), stream()), "seq_whiten_bwd")
            _check(f"whiten bwd {dtype} ldo={ldo}", dx[:B * N, :C].float().reshape(B, NC), dx_r, edx, dtype == BF)
            assert torch.isnan(dx[:B * N, C:]).all() and torch.isnan(dx[B * N]).all()
    dx = torch.full((B * N, C), 7.0, device="cuda")
    assert lib.htrvt_seq_whiten_bwd(ptr(dy_d), ptr(y_d), ptr(st_d), ptr(dx), B, N, C, C - 1, 0, stream()) != 0
    torch.cuda.synchronize()
    assert (dx == 7).all()


# ====================================================================== BatchNorm statistics
@pytest.mark.parametrize("C", [8, 64, 100, 192])
@pytest.mark.parametrize("rows", [1, 17, 256, 257, 1000])
def test_bn_finalize(rows, C):
    """partial sums -> scale / shift / saved statistics / running statistics; above 256 rows the two-level path, which
    uses the 64 rows behind the partial rows as scratch (and nothing behind those); a channel of variance 0"""
    lib, check, ptr, stream, dt, _ = _lib()
    g = _gen(rows * 1000 + C)
    ppr = 16                                               # pixels per partial row
    mu, sd = torch.rand(C, generator=g) * 4 - 2, torch.rand(C, generator=g) * 1.5 + 0.5
    x = (torch.randn(rows, ppr, C, generator=g) * sd + mu).double()
    x[:, :, 3] = 1.5                                       # variance exactly 0: rstd = 1 / sqrt(eps)
    partial = torch.stack([x.sum(1), (x * x).sum(1)], dim=1).float()          # [rows][2][C], the kernel's input
    count = float(rows * ppr)
    gamma, beta = torch.randn(C, generator=g) + 1, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    mom = 0.1
    with_running = (rows + C) % 2 == 0 or rows == 1
    print(f"\nbn_finalize rows={rows} C={C} running={with_running}")
    args = [partial, gamma, beta] + ([rm0, rv0] if with_running else [])
    ref, errs = R.e32(lambda p, ga, be, rm=None, rv=None: R.bn_finalize(p, count, ga, be, EPS_BN, mom, rm, rv), args)

    scratch = 64 if rows > 256 else 0
    buf = torch.full((rows + scratch + 4, 2, C), float("nan"), device="cuda")
    buf[:rows] = partial.cuda()
    gamma_d, beta_d = gamma.cuda(), beta.cuda()
    rm, rv = rm0.cuda(), rv0.cuda()
    nbt = torch.tensor([41], dtype=torch.int64, device="cuda")
    out = torch.full((4, C + 1), 7.0, device="cuda")      # scale, shift, mean, rstd (+ one guard column each)
    outs = [out[i] for i in range(4)]
    check(lib.htrvt_bn_finalize(ptr(buf), rows, C, count, ptr(gamma_d), ptr(beta_d), EPS_BN, mom,
                                ptr(rm) if with_running else None, ptr(rv) if with_running else None,
                                ptr(nbt) if with_running else None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), stream()),
          "bn_finalize")
    for i, name in enumerate(("scale", "shift", "mean", "rstd")):
        _check(name, outs[i][:C], ref[i], errs[i], False)
    assert (out[:, C] == 7).all()
    assert torch.isnan(buf[rows + scratch:]).all() and torch.equal(buf[:rows].cpu(), partial)
    assert abs(float(outs[3][3]) * EPS_BN ** 0.5 - 1.0) < 1e-6           # the variance-0 channel
    if with_running:
        _check("running_mean", rm, ref[4], errs[4], False)
        _check("running_var", rv, ref[5], errs[5], False)
        assert int(nbt) == 42
    else:
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 41


def test_bn_finalize_with_one_element_per_channel_keeps_the_biased_variance():
    """count = 1: there is no unbiased variance (torch: NaN); include/htrvt.h states that running_var then takes the
    biased one, 0 -- exact on integer data"""
    lib, check, ptr, stream, dt, _ = _lib()
    C = 8
    v = torch.arange(-3, 5).float()
    partial = torch.stack([v, v * v])[None].contiguous().cuda()
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    rm, rv = torch.full((C,), 2.0, device="cuda"), torch.full((C,), 4.0, device="cuda")
    scale, shift, mean, rstd = (torch.empty(C, device="cuda") for _ in range(4))
    check(lib.htrvt_bn_finalize(ptr(partial), 1, C, 1.0, ptr(one), ptr(zero), EPS_BN, 0.5, ptr(rm), ptr(rv), None, ptr(scale),
                                ptr(shift), ptr(mean), ptr(rstd), stream()), "bn_finalize")
    assert torch.equal(mean.cpu(), v) and torch.equal(rm.cpu(), 1.0 + 0.5 * v) and torch.equal(rv.cpu(), torch.full((C,), 2.0))
    want = R.bn_finalize(partial.cpu().double(), 1.0, one.cpu().double(), zero.cpu().double(), EPS_BN, 0.5)[3]
    assert ((rstd.cpu().double() - want).abs() <= 2.0 ** -23 * want).all()


@pytest.mark.parametrize("C", [8, 100])
def test_bn_eval_coeffs(C):
    lib, check, ptr, stream, dt, _ = _lib()
    g = _gen(C)
    gamma, beta = torch.randn(C, generator=g) + 1, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) * 3 + 0.01
    print(f"\nbn_eval_coeffs C={C}")
    ref, errs = R.e32(lambda a, b, c, d: R.bn_eval_coeffs(a, b, c, d, EPS_BN), [gamma, beta, rm, rv])
    gd, bd, rmd, rvd = gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda()
    for with_rstd in (True, False):
        out = torch.full((3, C + 1), 7.0, device="cuda")
        check(lib.htrvt_bn_eval_coeffs(ptr(gd), ptr(bd), ptr(rmd), ptr(rvd), EPS_BN, ptr(out[0]), ptr(out[1]),
                                       ptr(out[2]) if with_rstd else None, C, stream()), "bn_eval_coeffs")
        _check("eval scale", out[0, :C], ref[0], errs[0], False)
        _check("eval shift", out[1, :C], ref[1], errs[1], False)
        if with_rstd:
            _check("eval rstd", out[2, :C], ref[2], errs[2], False)
        else:
            assert (out[2] == 7).all()
        assert (out[:, C] == 7).all()


# ====================================================================== BatchNorm apply (exact)
def _mask_bits(y):
    w = (1 << torch.arange(8, device=y.device)).to(torch.int32)
    return ((y.reshape(-1, 8) > 0).to(torch.int32) * w).sum(1).to(torch.uint8)


def _apply_case(lib, check, ptr, stream, dt, dtype, npix, C, mode, relu, seed, with_mask, chunk=1 << 16):
    """integer data in [-8, 8], coefficients from {+-1/2, +-1, +-2}, integer shifts: every product and sum is exact in
    float32 and the result (|.| <= 40, a multiple of 1/2) in bfloat16, whatever the evaluation order"""
    torch.manual_seed(seed)
    dev = "cuda"
    x = torch.randint(-8, 9, (npix, C), device=dev).to(dtype)
    res = torch.randint(-8, 9, (npix, C), device=dev).to(dtype) if mode else None
    g = _gen(seed)
    sc, sf = _pick(g, C).cuda(), _ints(g, -4, 4, C).cuda()
    rsc, rsf = (_pick(g, C).cuda(), _ints(g, -4, 4, C).cuda()) if mode == 2 else (None, None)
    y = torch.full((npix + 1, C), 99.0, dtype=dtype, device=dev)
    if with_mask:
        mask = torch.full((npix * C // 8 + 8,), 0xAA, dtype=torch.uint8, device=dev)
        check(lib.htrvt_bn_apply_mask(ptr(x), ptr(sc), ptr(sf), ptr(res), ptr(rsc), ptr(rsf), ptr(y), ptr(mask), npix, C, relu,
                                      dt(dtype), stream()), "bn_apply_mask")
    else:
        check(lib.htrvt_bn_apply(ptr(x), ptr(sc), ptr(sf), ptr(res), ptr(rsc), ptr(rsf), ptr(y), npix, C, relu, dt(dtype), stream()),
              "bn_apply")
    for p0 in range(0, npix, chunk):
        sl = slice(p0, min(npix, p0 + chunk))
        want = R.bn_apply(x[sl].float(), sc, sf, None if res is None else res[sl].float(), rsc, rsf, bool(relu))
        assert torch.equal(y[sl].float(), want), (npix, C, mode, relu, p0)
        if with_mask:
            assert torch.equal(mask[p0 * C // 8:sl.stop * C // 8], _mask_bits(want)), (npix, C, mode, relu, p0)
    assert (y[npix] == 99).all()
    if with_mask:
        assert (mask[npix * C // 8:] == 0xAA).all()
    del x, res, y


APPLY_CASES = [(d, C, n) for d, C in ((BF, 8), (BF, 24), (BF, 192), (BF, 384), (F32, 4), (F32, 12), (F32, 192)) for n in (1, 37, 65541)]
APPLY_CASES += [(BF, 24, 200001), (F32, 12, 200001)]


@pytest.mark.parametrize("dtype,C,npix", APPLY_CASES)
def test_bn_apply_is_exact_on_representable_data(dtype, C, npix):
    """residual modes x ReLU; 65 541 pixels with 24 / 48 channel vectors and 200 001 with 3 are past the grid cap of
    2 048 x 256 threads, where threads loop and the channel index advances by a non-zero step"""
    lib, check, ptr, stream, dt, _ = _lib()
    for mode in (0, 1, 2):
        for relu in (0, 1):
            _apply_case(lib, check, ptr, stream, dt, dtype, npix, C, mode, relu, npix + C + mode, False)
            if dtype == BF:
                _apply_case(lib, check, ptr, stream, dt, dtype, npix, C, mode, relu, npix + C + mode, True)


@pytest.mark.parametrize("mode,with_mask", [(0, False), (2, False), (1, True)])
def test_bn_apply_streaming_instances(mode, with_mask):
    """tensors of at least 150 MiB take the non-temporal-load instances"""
    lib, check, ptr, stream, dt, _ = _lib()
    C, npix = 192, 425003
    assert npix * C * 2 >= 150 << 20
    _apply_case(lib, check, ptr, stream, dt, BF, npix, C, mode, 1, 11 + mode, with_mask)
    torch.cuda.empty_cache()


# ====================================================================== BatchNorm backward
def _bwd_apply_cases(lib, check, ptr, stream, dt, dtype, npix, C, seed, chunk=1 << 16):
    """bn_bwd_apply (yact NULL / given, gout NULL / given) and bn_bwd_apply2, exact: coefficients from the set, integer
    constants and data"""
    torch.manual_seed(seed)
    dev = "cuda"
    g = _gen(seed)
    dy = torch.randint(-8, 9, (npix, C), device=dev).to(dtype)
    x = torch.randint(-8, 9, (npix, C), device=dev).to(dtype)
    x2 = torch.randint(-8, 9, (npix, C), device=dev).to(dtype)
    yact = torch.randint(-2, 3, (npix, C), device=dev).to(dtype)                 # exact zeros and negatives: both closed
    coef = torch.stack([_pick(g, C), _pick(g, C), _ints(g, -4, 4, C)]).cuda()
    coef2 = torch.stack([_pick(g, C), _pick(g, C), _ints(g, -4, 4, C)]).cuda()

    def chunks():
        for p0 in range(0, npix, chunk):
            yield slice(p0, min(npix, p0 + chunk))

    for with_act in (False, True):
        for with_gout in (False, True):
            dx = torch.full((npix + 1, C), 99.0, dtype=dtype, device=dev)
            gout = torch.full((npix + 1, C), 99.0, dtype=dtype, device=dev)
            check(lib.htrvt_bn_bwd_apply(ptr(dy), ptr(yact) if with_act else None, ptr(x), ptr(coef), ptr(dx),
                                         ptr(gout) if with_gout else None, npix, C, dt(dtype), stream()), "bn_bwd_apply")
            for sl in chunks():
                gm = dy[sl].float() if not with_act else torch.where(yact[sl].float() > 0, dy[sl].float(), torch.zeros((), device=dev))
                assert torch.equal(dx[sl].float(), coef[0] * gm + coef[1] * x[sl].float() + coef[2]), (npix, C, with_act, sl.start)
                if with_gout:
                    assert torch.equal(gout[sl].float(), gm)
            assert (dx[npix] == 99).all() and (gout[npix if with_gout else 0] == 99).all()
            del dx, gout
    dx1 = torch.full((npix + 1, C), 99.0, dtype=dtype, device=dev)
    dx2 = torch.full((npix + 1, C), 99.0, dtype=dtype, device=dev)
    check(lib.htrvt_bn_bwd_apply2(ptr(dy), ptr(x), ptr(coef), ptr(dx1), ptr(x2), ptr(coef2), ptr(dx2), npix, C, dt(dtype), stream()),
          "bn_bwd_apply2")
    for sl in chunks():
        gm = dy[sl].float()
        assert torch.equal(dx1[sl].float(), coef[0] * gm + coef[1] * x[sl].float() + coef[2]), (npix, C, sl.start)
        assert torch.equal(dx2[sl].float(), coef2[0] * gm + coef2[1] * x2[sl].float() + coef2[2]), (npix, C, sl.start)
    assert (dx1[npix] == 99).all() and (dx2[npix] == 99).all()


# channel vectors per pixel: 1, 3, 24 (256 % 24 != 0: idle threads in the reduction), 48, 256 (the limit)
BWD_C = [(BF, 8), (BF, 24), (BF, 192), (BF, 384), (BF, 2048), (F32, 4), (F32, 12), (F32, 96), (F32, 192), (F32, 1024)]


@pytest.mark.parametrize("npix", [1, 37, 63, 64, 65541])
@pytest.mark.parametrize("dtype,C", BWD_C)
def test_bn_backward_reduce_and_apply_are_exact_on_representable_data(dtype, C, npix):
    """bn_bwd_reduce with integer mean, rstd in {1/2, 1, 2} and integer data (|sum| <= 192 * 65 541 = 1.26e7 < 2^24:
    every partial and total is exact), its partial rows summed directly and through colsum; dgamma / dbeta accumulate
    exactly; eval-mode coefficients exact; then the apply kernels.  65 541 pixels are past the 1 024-block cap of the
    reduction and, with 24 / 48 channel vectors, past the grid cap of the apply kernels."""
    lib, check, ptr, stream, dt, colsum = _lib()
    ch = 8 if dtype == BF else 4
    if C // ch == 256 and npix == 65541:
        npix = 2100                                        # 33 partial rows; the full count would be 1 GiB of operands
    torch.manual_seed(npix + C)
    g = _gen(npix * 3 + C)
    dev = "cuda"
    dy = torch.randint(-8, 9, (npix, C), device=dev).to(dtype)
    x = torch.randint(-8, 9, (npix, C), device=dev).to(dtype)
    yact = torch.randint(-2, 3, (npix, C), device=dev).to(dtype)
    mean, rstd = _ints(g, -4, 4, C).cuda(), _pick(g, C, (0.5, 1.0, 2.0)).cuda()
    gamma = _pick(g, C).cuda()
    nblk = lib.htrvt_bn_bwd_blocks(npix)
    assert nblk == max(1, min(npix // 64, 1024))
    for with_act in (False, True):
        partial = torch.full((nblk + 1, 2, C), 99.0, device=dev)
        check(lib.htrvt_bn_bwd_reduce(ptr(dy), ptr(yact) if with_act else None, ptr(x), ptr(mean), ptr(rstd), ptr(partial), npix, C,
                                      dt(dtype), stream()), "bn_bwd_reduce")
        _, s1, s2 = R.bn_bwd_sums(dy.double(), yact.double() if with_act else None, x.double(), mean.double(), rstd.double())
        assert (partial[nblk] == 99).all()
        assert torch.equal(partial[:nblk, 0].double().sum(0), s1) and torch.equal(partial[:nblk, 1].double().sum(0), s2)
        # finalize: directly over the rows, and over one row made by colsum (Engine.bn_backward_coef above 64 rows)
        red = torch.zeros(2 * C, device=dev)
        colsum(partial, nblk, 2 * C, 2 * C, red, dti=0)
        assert torch.equal(red.double(), torch.cat([s1, s2]))
        for src, rows in ((partial, nblk), (red, 1)):
            for count in (float(npix), -1.0):
                dgb = _ints(g, -5, 5, 2, C).cuda()
                dgb0 = dgb.clone()
                coef = torch.full((3 * C + 1,), 99.0, device=dev)
                check(lib.htrvt_bn_bwd_finalize(ptr(src), rows, C, count, ptr(gamma), ptr(mean), ptr(rstd), ptr(dgb[0]), ptr(dgb[1]),
                                                ptr(coef), stream()), "bn_bwd_finalize")
                assert torch.equal(dgb[0].double(), dgb0[0].double() + s2) and torch.equal(dgb[1].double(), dgb0[1].double() + s1)
                assert coef[3 * C] == 99
                want = R.bn_bwd_coef(s1, s2, count, gamma.double(), mean.double(), rstd.double())
                got = coef[:3 * C].view(3, C)
                assert torch.equal(got[0], want[0].float())          # gamma * rstd: exact
                if count <= 0:
                    assert not got[1:].any()
                else:       # a division by count: double arithmetic (2^-45 of the terms that may cancel in cC), one rounding
                    slack = torch.zeros_like(want)
                    slack[2] = 2.0 ** -45 * ((want[0] * s1 / count).abs() + (want[1] * mean.double()).abs())
                    assert ((got.double() - want).abs() <= 2.0 ** -23 * want.abs() + slack).all()
    del partial
    _bwd_apply_cases(lib, check, ptr, stream, dt, dtype, npix, C, npix + C)


def test_bn_backward_apply_streaming_instances():
    lib, check, ptr, stream, dt, _ = _lib()
    C, npix = 192, 425003
    assert npix * C * 2 >= 150 << 20
    _bwd_apply_cases(lib, check, ptr, stream, dt, BF, npix, C, 5)
    torch.cuda.empty_cache()


CHAIN_CASES = [(d, C, n) for d, C in ((BF, 24), (BF, 384), (F32, 12), (F32, 96)) for n in (37, 4099)] + [(BF, 24, 65541), (F32, 12, 65541)]


@pytest.mark.parametrize("dtype,C,npix", CHAIN_CASES)
def test_bn_backward_chain_against_float64(dtype, C, npix):
    """reduce -> finalize (train) -> apply on real-valued data: dx, dgamma, dbeta and the coefficients against the float64
    closed form over the same inputs, and against float64 autograd over F.batch_norm"""
    lib, check, ptr, stream, dt, _ = _lib()
    g = _gen(npix + C)
    bf = dtype == BF
    mu, sd = torch.rand(C, generator=g) * 4 - 2, torch.rand(C, generator=g) * 1.5 + 0.5
    x = (torch.randn(npix, C, generator=g) * sd + mu).to(dtype)
    dy = torch.randn(npix, C, generator=g).to(dtype)
    gamma, beta = torch.randn(C, generator=g) + 1, torch.randn(C, generator=g)
    xd = x.double()
    mean64 = xd.mean(0)
    mean, rstd = mean64.float(), (1.0 / torch.sqrt(((xd - mean64) ** 2).mean(0) + EPS_BN)).float()     # inputs of the kernels
    scale = gamma * rstd
    yact = torch.relu(x.float() * scale + (beta - mean * scale)).to(dtype)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    count = float(npix)
    print(f"\nbn backward {dtype} C={C} npix={npix}")
    dy_d, x_d, yact_d, mean_d, rstd_d, gamma_d = dy.cuda(), x.cuda(), yact.cuda(), mean.cuda(), rstd.cuda(), gamma.cuda()
    nblk = lib.htrvt_bn_bwd_blocks(npix)
    for with_act in (False, True):
        def ref(dy_, ya_, x_, m_, r_, ga_, dg0_, db0_):
            dx_, dga_, dbe_, g_ = R.bn_bwd(dy_, ya_ if with_act else None, x_, m_, r_, ga_, count)
            _, s1_, s2_ = R.bn_bwd_sums(dy_, ya_ if with_act else None, x_, m_, r_)
            return dx_, dga_ + dg0_, dbe_ + db0_, R.bn_bwd_coef(s1_, s2_, count, ga_, m_, r_)
        (dx_r, dg_r, db_r, coef_r), (edx, edg, edb, eco) = R.e32(ref, [dy.float(), yact.float(), x.float(), mean, rstd, gamma, dg0, db0])
        partial = torch.empty(nblk, 2, C, device="cuda")
        dgb = torch.stack([dg0, db0]).cuda()
        coef = torch.empty(3, C, device="cuda")
        dx = torch.empty(npix, C, dtype=dtype, device="cuda")
        act_p = ptr(yact_d) if with_act else None
        check(lib.htrvt_bn_bwd_reduce(ptr(dy_d), act_p, ptr(x_d), ptr(mean_d), ptr(rstd_d), ptr(partial), npix, C, dt(dtype), stream()),
              "bn_bwd_reduce")
        check(lib.htrvt_bn_bwd_finalize(ptr(partial), nblk, C, count, ptr(gamma_d), ptr(mean_d), ptr(rstd_d), ptr(dgb[0]), ptr(dgb[1]),
                                        ptr(coef), stream()), "bn_bwd_finalize")
        check(lib.htrvt_bn_bwd_apply(ptr(dy_d), act_p, ptr(x_d), ptr(coef), ptr(dx), None, npix, C, dt(dtype), stream()), "bn_bwd_apply")
        tag = "masked" if with_act else "plain"
        _check(f"{tag} dx", dx.float(), dx_r, edx, bf)
        _check(f"{tag} dgamma", dgb[0], dg_r, edg, False)
        _check(f"{tag} dbeta", dgb[1], db_r, edb, False)
        _check(f"{tag} coef", coef, coef_r, eco, False)
        if not with_act:                                   # float64 autograd with its own batch statistics
            def auto(dy_, x_, ga_, be_, dg0_, db0_):
                dx_, dga_, dbe_, _, _ = R.bn_bwd_autograd(dy_, x_, ga_, be_, EPS_BN)
                return dx_, dga_ + dg0_, dbe_ + db0_
            (dxa, dga, dba), errs = R.e32(auto, [dy.float(), x.float(), gamma, beta, dg0, db0])
            _check("autograd dx", dx.float(), dxa, errs[0], bf)
            _check("autograd dgamma", dgb[0], dga, errs[1], False)
            _check("autograd dbeta", dgb[1], dba, errs[2], False)


def test_bn_backward_refuses_unsupported_widths_without_launching():
    lib, check, ptr, stream, dt, _ = _lib()
    npix = 4
    for fn, dtype, C in (("reduce", F32, 1028), ("reduce", BF, 2056), ("apply2", BF, 2056), ("apply2", F32, 2052), ("apply", BF, 12),
                         ("reduce", F32, 6)):
        x = torch.ones(npix, C, dtype=dtype, device="cuda")
        vec = torch.ones(3 * C, device="cuda")
        out = torch.full((npix, C), 7.0, dtype=dtype, device="cuda")
        part = torch.full((1, 2, C), 7.0, device="cuda")
        if fn == "reduce":
            rc = lib.htrvt_bn_bwd_reduce(ptr(x), None, ptr(x), ptr(vec), ptr(vec), ptr(part), npix, C, dt(dtype), stream())
        elif fn == "apply":
            rc = lib.htrvt_bn_bwd_apply(ptr(x), None, ptr(x), ptr(vec), ptr(out), None, npix, C, dt(dtype), stream())
        else:
            rc = lib.htrvt_bn_bwd_apply2(ptr(x), ptr(x), ptr(vec), ptr(out), ptr(x), ptr(vec), ptr(out), npix, C, dt(dtype), stream())
        torch.cuda.synchronize()
        assert rc != 0 and (out == 7).all() and (part == 7).all(), (fn, dtype, C)
