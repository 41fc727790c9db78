"""The convolutional token mixer on the MI355X: csrc/mixer.hip through the C ABI against tests/conv_mixer_refs.py in
float64, the autograd wrapper variants.glu_dwconv_bn_silu, and htrvt_amd.mixer.ConvLocalMixer1D against
tests/golden/conv_mixer.npz (the fork's own module in float64).

Kernel gates follow tests/test_norm_kernels_gpu.py: per element against the float64 reference over the same (already
rounded) inputs, relative to the reference's largest magnitude, gate = 8 * E32 (+ 2^-8 |ref| for a bfloat16 output) with
E32 = kernel_refs.e32, the float32 evaluation error of the reference itself on these inputs.  Nothing in a gate comes from
the kernel under test.  The launches are checked stage by stage, a later stage's reference taking the earlier launches'
outputs as its inputs (c as stored, the per-channel coefficients), as the kernels do.  Every comparison prints E32, gate
and observed error (`pytest -s`).

Measured on an MI355X, over all parametrised cases of an output (errors relative to max |ref|; a bfloat16 gate is
2^-8 = 3.9e-3 plus 8 * E32):

  output                         E32 (range)        worst observed   worst observed / gate
  c                     bf16     7.0e-8 .. 1.5e-7   2.8e-3           0.72
  c                     f32      6.1e-8 .. 1.6e-7   1.6e-7           0.20
  stats scale / shift            2.5e-8 .. 6.8e-5   3.6e-5           0.22 / 0.39   (N = 2, k = 1: variance 1e-3 of mean^2)
  stats mean / rstd              0 .. 6.8e-5        1.1e-7 / 3.6e-5  0.23 / 0.16
  stats running_mean / _var      1.3e-8 .. 1.0e-7   8.3e-8 / 1.0e-7  0.13
  s                     bf16     4.8e-8 .. 4.0e-7   2.9e-3           0.74
  s                     f32      4.2e-8 .. 7.7e-7   1.2e-7           0.13
  sum dz / sum dz xhat           2.9e-8 .. 2.4e-7   2.9e-7 / 2.3e-7  0.39 / 0.32
  du                    bf16     4.6e-8 .. 1.3e-5   3.2e-3           0.83
  du                    f32      4.1e-8 .. 1.4e-5   2.5e-7           0.17
  dw / dbias                     4.3e-8 .. 3.3e-4   1.7e-5 / 1.4e-7  0.36 / 0.17
  variants wrapper, f32: s, du   1.1e-7 .. 1.7e-7   1.7e-7           0.13
    dw, dgamma, dbeta, dbias     3.0e-8 .. 3.2e-7   3.3e-7           0.35
    running_mean / running_var   4.9e-8 .. 6.4e-8   7.4e-8           0.14
  module, float32: outputs and buffers 1.7e-7 (gate 1e-3), gradients 7.9e-7 (gate 2e-3)
  module, bfloat16: outputs 3.5e-3, buffers 5.4e-5 (gate 5e-2), gradients 9.4e-3 (gate 1e-1)
  dropout p = 0.1: dropped share 0.0990 of 6335 unambiguous elements; gradients with the recovered mask 5.8e-7
"""
import os

import numpy as np
import pytest
import torch

import conv_mixer_cases as C
import conv_mixer_refs as M
import kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
EPS = float(torch.tensor(1e-5, dtype=F32))
MOM = float(torch.tensor(0.1, dtype=F32))
SHAPES = [(2, 5, 8, 7), (3, 33, 24, 7), (2, 16, 64, 3), (2, 16, 64, 9), (2, 128, 768, 7), (1, 2, 8, 1)]


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import colsum, dt, ptr, stream
    return lib, check, ptr, stream, dt, colsum


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, got, ref, err, bf16_out):
    ok, obs = R.gate_check(name, got.detach().cpu(), ref, err, bf16_out)
    assert ok, f"{name}: observed {obs:.3e} of max|ref| is outside 8 * E32 = {8 * err:.3e}" + (" + one bf16 ulp" if bf16_out else "")


def _inputs(B, N, D, k, dtype, seed):
    g = _gen(seed)
    u = (torch.randn(B * N, 2 * D, generator=g) * 1.5).to(dtype)
    ds = torch.randn(B * N, D, generator=g).to(dtype)
    w = torch.randn(D, k, generator=g) * 0.4
    gamma, beta = torch.randn(D, generator=g) * 0.3 + 1, torch.randn(D, generator=g) * 0.3
    rm, rv = torch.randn(D, generator=g) * 0.3, torch.rand(D, generator=g) + 0.5
    bias = torch.randn(D, generator=g) * 0.3
    return u, ds, w, gamma, beta, rm, rv, bias


def _stats_ref(c, gamma, beta, rm, rv):
    """what htrvt_bn_finalize makes of the partial rows of c"""
    partial = torch.stack([c.sum(0), (c * c).sum(0)])[None]
    return R.bn_finalize(partial, float(c.shape[0]), gamma, beta, EPS, MOM, rm, rv)


# ====================================================================== the launches, stage by stage
@pytest.mark.parametrize("mode", ["train", "eval", "nobn"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,N,D,k", SHAPES)
def test_kernels_against_float64(B, N, D, k, dtype, mode):
    lib, check, ptr, stream, dt, colsum = _lib()
    bf, dti, rows = dtype == BF, dt(dtype), B * N
    u, ds, w, gamma, beta, rm, rv, bias = _inputs(B, N, D, k, dtype, 31 * N + D + k)
    print(f"\nmixer {mode} {dtype} B={B} N={N} D={D} k={k}")
    dev = {n: t.cuda() for n, t in dict(u=u, ds=ds, w=w, gamma=gamma, beta=beta, rm=rm, rv=rv, bias=bias).items()}
    vec = lambda: torch.full((D,), 7.0, device="cuda")                      # noqa: E731
    c = torch.full((rows + 1, D), 7.0, dtype=dtype, device="cuda")
    s = torch.full((rows + 1, D), 7.0, dtype=dtype, device="cuda")
    scale, shift, mean, rstd = vec(), vec(), vec(), vec()
    nbt = torch.tensor(5, dtype=torch.int64, device="cuda")

    # ---- forward
    if mode == "train":
        R_ = lib.htrvt_mixer_rows(B, N, D, dti)
        nws = lib.htrvt_mixer_fwd_workspace_floats(B, N, D, dti)
        assert R_ >= 1 and nws == (R_ + 64) * 2 * D
        partial = torch.full((nws + 1,), 7.0, device="cuda")
        check(lib.htrvt_mixer_fwd_train(ptr(dev["u"]), ptr(dev["w"]), ptr(c), ptr(partial), B, N, D, k, dti, stream()), "fwd_train")
        assert partial[nws] == 7
        check(lib.htrvt_bn_finalize(ptr(partial), R_, D, float(rows), ptr(dev["gamma"]), ptr(dev["beta"]), EPS, MOM, ptr(dev["rm"]),
                                    ptr(dev["rv"]), ptr(nbt), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), stream()), "bn_finalize")
        check(lib.htrvt_mixer_bn_silu(ptr(c), ptr(scale), ptr(shift), ptr(s), rows, D, dti, stream()), "bn_silu")
        ck = c[:rows].float().cpu()
        ref, errs = R.e32(_stats_ref, [ck, gamma, beta, rm, rv])
        got = (scale, shift, mean, rstd, dev["rm"], dev["rv"])
        for n, g_, r_, e_ in zip(("scale", "shift", "mean", "rstd", "running_mean", "running_var"), got, ref, errs):
            _check("stats " + n, g_, r_, e_, False)
        assert int(nbt) == 6
    else:
        if mode == "eval":
            check(lib.htrvt_bn_eval_coeffs(ptr(dev["gamma"]), ptr(dev["beta"]), ptr(dev["rm"]), ptr(dev["rv"]), EPS, ptr(scale),
                                           ptr(shift), ptr(rstd), D, stream()), "bn_eval_coeffs")
            mean = dev["rm"]
            sc_p, sh_p = ptr(scale), ptr(shift)
        else:
            scale, shift, sc_p, sh_p = None, dev["bias"], None, ptr(dev["bias"])
        check(lib.htrvt_mixer_fwd_eval(ptr(dev["u"]), ptr(dev["w"]), sc_p, sh_p, ptr(c), ptr(s), B, N, D, k, dti, stream()), "fwd_eval")
        s2 = torch.empty(rows, D, dtype=dtype, device="cuda")
        check(lib.htrvt_mixer_fwd_eval(ptr(dev["u"]), ptr(dev["w"]), sc_p, sh_p, None, ptr(s2), B, N, D, k, dti, stream()),
              "fwd_eval without c")
        assert torch.equal(s2, s[:rows])
        assert torch.equal(dev["rm"].cpu(), rm) and torch.equal(dev["rv"].cpu(), rv)
    (c_r,), (ec,) = R.e32(lambda a, b: M.glu_dwconv(a, b, B, N), [u.float(), w])
    _check("c", c[:rows].float(), c_r, ec, bf)
    ck = c[:rows].float().cpu()
    sc_h = None if scale is None else scale.cpu()
    sh_h = shift.cpu()
    (s_r,), (es,) = R.e32(lambda a, b, d: M.silu(M.affine(a, b, d)), [ck, sc_h, sh_h])
    _check("s", s[:rows].float(), s_r, es, bf)
    assert (c[rows] == 7).all() and (s[rows] == 7).all()

    # ---- backward
    coef = None
    if mode != "nobn":
        Q = lib.htrvt_mixer_reduce_rows(rows, D, dti)
        assert 1 <= Q <= 128
        part = torch.full((Q + 1, 2, D), 7.0, device="cuda")
        check(lib.htrvt_mixer_bwd_reduce(ptr(dev["ds"]), ptr(c), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(part), rows, D,
                                         dti, stream()), "bwd_reduce")
        assert (part[Q] == 7).all()
        mean_h, rstd_h = mean.cpu(), rstd.cpu()
        (s1_r, s2_r), (e1, e2) = R.e32(M.bwd_sums, [ds.float(), ck, sc_h, sh_h, mean_h, rstd_h])
        sums = part[:Q].double().sum(0).cpu()
        _check("sum dz", sums[0], s1_r, e1, False)
        _check("sum dz xhat", sums[1], s2_r, e2, False)
        coef, dgam, dbet = torch.empty(3, D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        check(lib.htrvt_bn_bwd_finalize(ptr(part), Q, D, float(rows) if mode == "train" else 0.0, ptr(dev["gamma"]), ptr(mean),
                                        ptr(rstd), ptr(dgam), ptr(dbet), ptr(coef), stream()), "bn_bwd_finalize")
    R_ = lib.htrvt_mixer_rows(B, N, D, dti)
    assert lib.htrvt_mixer_bwd_workspace_floats(B, N, D, k, dti) == R_ * D * (k + 1)
    pw = torch.full((R_ + 1, D * k), 7.0, device="cuda")
    pb = torch.full((R_ + 1, D), 7.0, device="cuda") if mode == "nobn" else None
    du = torch.full((rows + 1, 2 * D), 7.0, dtype=dtype, device="cuda")
    check(lib.htrvt_mixer_bwd(ptr(dev["u"]), ptr(c), ptr(dev["ds"]), ptr(dev["w"]), None if scale is None else ptr(scale), ptr(shift),
                              None if coef is None else ptr(coef), ptr(du), ptr(pw), None if pb is None else ptr(pb), B, N, D, k,
                              dti, stream()), "mixer_bwd")
    dw = torch.zeros(D, k, device="cuda")
    colsum(pw, R_, D * k, D * k, dw, dti=0)
    coef_h = None if coef is None else coef.cpu()
    (du_r, dw_r, db_r), (edu, edw, edb) = R.e32(lambda *a: M.core_bwd(*a[:4], B, N, *a[4:]), [ds.float(), ck, u.float(), w, sc_h, sh_h, coef_h])
    _check("du", du[:rows].float(), du_r, edu, bf)
    _check("dw", dw, dw_r, edw, False)
    assert (du[rows] == 7).all() and (pw[R_] == 7).all()
    if pb is not None:
        db = torch.zeros(D, device="cuda")
        colsum(pb, R_, D, D, db, dti=0)
        _check("dbias", db, db_r, edb, False)
        assert (pb[R_] == 7).all()


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_images_do_not_see_each_other(dtype):
    """eval mode: changing image 1's u leaves image 0's c, s and du bit for bit"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    B, N, D, k = 2, 5, 8, 7
    u, ds, w, gamma, beta, rm, rv, _ = [t.cuda() for t in _inputs(B, N, D, k, dtype, 3)]
    w = w.view(D, 1, k).contiguous()
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    u2 = u.clone()
    u2[N:] = (u2[N:].float() * -3 + 1).to(dtype)
    out = []
    for uu in (u, u2):
        s, saved = seq_ops.conv_mixer_fwd(uu, w, B, N, bn=(gamma, beta, rm, rv, nbt), training=False, eps=EPS)
        du = seq_ops.conv_mixer_bwd(ds, uu, w, B, N, saved, gamma=gamma, training=False)[0]
        out.append((saved[0], s, du))
    for a, b in zip(*out):
        assert torch.equal(a[:N], b[:N])
        assert not torch.equal(a[N:], b[N:])


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,N,D,k", [(2, 5, 8, 7), (3, 33, 24, 7), (2, 16, 64, 9)])
def test_exact_case(B, N, D, k, dtype):
    """integer-valued g (gate half 30: sigmoid is exactly 1 in float32) and taps from {+-0.5, +-1, +-2}: every product and
    partial sum is representable, c equals the reference bit for bit"""
    lib, check, ptr, stream, dt, _ = _lib()
    g = _gen(N + k)
    a = torch.randint(-4, 5, (B * N, D), generator=g).float()
    u = torch.cat([a, torch.full((B * N, D), 30.0)], 1).to(dtype)
    w = torch.tensor((-2.0, -1.0, -0.5, 0.5, 1.0, 2.0))[torch.randint(0, 6, (D, k), generator=g)]
    ref = M.dwconv_tokens(a.double(), w.double(), B, N)
    assert torch.equal(ref.to(dtype).double(), ref)
    u_d, w_d = u.cuda(), w.cuda()
    c = torch.empty(B * N, D, dtype=dtype, device="cuda")
    s = torch.empty(B * N, D, dtype=dtype, device="cuda")
    check(lib.htrvt_mixer_fwd_eval(ptr(u_d), ptr(w_d), None, None, ptr(c), ptr(s), B, N, D, k, dt(dtype), stream()), "fwd_eval")
    assert torch.equal(c.double().cpu(), ref)
    part = torch.empty(lib.htrvt_mixer_fwd_workspace_floats(B, N, D, dt(dtype)), device="cuda")
    c2 = torch.empty_like(c)
    check(lib.htrvt_mixer_fwd_train(ptr(u_d), ptr(w_d), ptr(c2), ptr(part), B, N, D, k, dt(dtype), stream()), "fwd_train")
    assert torch.equal(c2, c)
    R_ = lib.htrvt_mixer_rows(B, N, D, dt(dtype))
    sums = part[:R_ * 2 * D].view(R_, 2, D).sum(0).double().cpu()      # sums of small multiples of 0.5 / 0.25: exact
    assert torch.equal(sums[0], ref.sum(0)) and torch.equal(sums[1], (ref * ref).sum(0))


def test_refusals_launch_nothing():
    lib, check, ptr, stream, dt, _ = _lib()
    B, N, D = 2, 6, 16
    for dtype in (BF, F32):
        dti = dt(dtype)
        u = torch.ones(B * N + 1, 2 * D, dtype=dtype, device="cuda")
        x = torch.ones(B * N + 1, D, dtype=dtype, device="cuda")
        out = torch.full((B * N + 1, D), 7.0, dtype=dtype, device="cuda")
        out2 = torch.full((B * N + 1, 2 * D), 7.0, dtype=dtype, device="cuda")
        w = torch.ones(D, 15, device="cuda")
        ws = torch.full((4096,), 7.0, device="cuda")
        vec = torch.ones(D, device="cuda")
        off = 4 if dtype == F32 else 2      # one element: no longer 16-byte aligned

        def all_three(u_p, c_p, o_p, o2_p, b, n, d, k):
            return (lib.htrvt_mixer_fwd_train(u_p, ptr(w), o_p, ptr(ws), b, n, d, k, dti, stream()),
                    lib.htrvt_mixer_fwd_eval(u_p, ptr(w), ptr(vec), ptr(vec), None, o_p, b, n, d, k, dti, stream()),
                    lib.htrvt_mixer_bwd(u_p, c_p, c_p, ptr(w), ptr(vec), ptr(vec), None, o2_p, ptr(ws), None, b, n, d, k, dti, stream()))
        bad = {"even k": all_three(ptr(u), ptr(x), ptr(out), ptr(out2), B, N, D, 6),
               "k = 0": all_three(ptr(u), ptr(x), ptr(out), ptr(out2), B, N, D, 0),
               "k = 17": all_three(ptr(u), ptr(x), ptr(out), ptr(out2), B, N, D, 17),
               "D = 12": all_three(ptr(u), ptr(x), ptr(out), ptr(out2), B, N, 12, 7),
               "u unaligned": all_three(ptr(u) + off, ptr(x), ptr(out), ptr(out2), B, N, D, 7),
               "out unaligned": all_three(ptr(u), ptr(x), ptr(out) + off, ptr(out2) + off, B, N, D, 7),
               "one row, train": (lib.htrvt_mixer_fwd_train(ptr(u), ptr(w), ptr(out), ptr(ws), 1, 1, D, 7, dti, stream()),)}
        bad["c unaligned"] = (lib.htrvt_mixer_bwd(ptr(u), ptr(x) + off, ptr(x), ptr(w), ptr(vec), ptr(vec), None, ptr(out2), ptr(ws),
                                                  None, B, N, D, 7, dti, stream()),
                              lib.htrvt_mixer_bwd(ptr(u), ptr(x), ptr(x) + off, ptr(w), ptr(vec), ptr(vec), None, ptr(out2), ptr(ws),
                                                  None, B, N, D, 7, dti, stream()))
        bad["bn_silu unaligned"] = (lib.htrvt_mixer_bn_silu(ptr(x) + off, ptr(vec), ptr(vec), ptr(out), B * N, D, dti, stream()),)
        bad["bwd_reduce unaligned"] = (lib.htrvt_mixer_bwd_reduce(ptr(x) + off, ptr(x), ptr(vec), ptr(vec), ptr(vec), ptr(vec),
                                                                  ptr(ws), B * N, D, dti, stream()),)
        bad["bwd_reduce D = 12"] = (lib.htrvt_mixer_bwd_reduce(ptr(x), ptr(x), ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(ws),
                                                               B * N, 12, dti, stream()),)
        for what, rcs in bad.items():
            assert all(rc < 0 for rc in rcs), (what, rcs)
        assert lib.htrvt_last_error()
        torch.cuda.synchronize()
        assert (out == 7).all() and (out2 == 7).all() and (ws == 7).all()
        assert lib.htrvt_mixer_rows(B, N, 12, dti) < 0 and lib.htrvt_mixer_fwd_workspace_floats(B, N, 12, dti) < 0


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("mode", ["train", "eval", "nobn"])
def test_two_calls_give_the_same_bits(mode, dtype):
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    B, N, D, k = 3, 33, 24, 7
    u, ds, w, gamma, beta, rm, rv, bias = [t.cuda() for t in _inputs(B, N, D, k, dtype, 11)]
    w = w.view(D, 1, k).contiguous()
    runs = []
    for _ in range(2):
        rm_, rv_, nbt = rm.clone(), rv.clone(), torch.zeros((), dtype=torch.int64, device="cuda")
        bn = None if mode == "nobn" else (gamma, beta, rm_, rv_, nbt)
        s, saved = seq_ops.conv_mixer_fwd(u, w, B, N, bn=bn, training=mode == "train", eps=EPS, momentum=MOM,
                                          conv_bias=bias if mode == "nobn" else None)
        grads = seq_ops.conv_mixer_bwd(ds, u, w, B, N, saved, gamma=None if mode == "nobn" else gamma, training=mode == "train",
                                       need_bias=mode == "nobn")
        runs.append([s, saved[0], rm_, rv_, nbt] + [g_ for g_ in grads if g_ is not None])
    assert len(runs[0]) == (8 if mode == "nobn" else 9)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ====================================================================== the autograd wrapper
@pytest.mark.parametrize("mode", ["train", "eval", "nobn"])
@pytest.mark.parametrize("B,N,D,k", [(2, 5, 8, 7), (3, 33, 24, 7)])
def test_variants_wrapper_against_float64_autograd(B, N, D, k, mode):
    """variants.glu_dwconv_bn_silu end to end in float32 against autograd through the float64 reference; gates from the
    reference's own float32 evaluation, as above"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import variants
    u, ds, w, gamma, beta, rm, rv, bias = _inputs(B, N, D, k, F32, 5 + N)
    train, bn = mode == "train", mode != "nobn"
    print(f"\nglu_dwconv_bn_silu {mode} B={B} N={N} D={D} k={k}")

    def ref(u_, w_, ga_, be_, rm_, rv_, bi_, ds_):
        kw = dict(gamma=ga_, beta=be_, running_mean=rm_, running_var=rv_) if bn else dict(conv_bias=bi_)
        s_, _, nrm, nrv = M.mixer_core(u_, w_, B, N, training=train, eps=EPS, momentum=MOM, **kw)
        g_ = M.mixer_core_bwd(ds_, u_, w_, B, N, training=train, eps=EPS, **kw)
        return (s_, g_["du"], g_["dw"], g_.get("dgamma"), g_.get("dbeta"), g_.get("dbias"), nrm, nrv)
    refs, errs = R.e32(ref, [u, w, gamma, beta, rm, rv, bias, ds])

    leaf = lambda t: t.cuda().requires_grad_(True)                        # noqa: E731
    ud, wd, gd, bd, bid = leaf(u), leaf(w.view(D, 1, k)), leaf(gamma), leaf(beta), leaf(bias)
    rmd, rvd, nbt = rm.cuda(), rv.cuda(), torch.tensor(3, dtype=torch.int64, device="cuda")
    if bn:
        s = variants.glu_dwconv_bn_silu(ud, wd, gd, bd, rmd, rvd, nbt, B, N, train, EPS, MOM)
    else:
        s = variants.glu_dwconv_bn_silu(ud, wd, None, None, None, None, None, B, N, train, EPS, MOM, conv_bias=bid)
    s.backward(ds.cuda())
    got = (s, ud.grad, wd.grad.view(D, k), gd.grad, bd.grad, bid.grad, rmd if train else None, rvd if train else None)
    for n, g_, r_, e_ in zip(("s", "du", "dw", "dgamma", "dbeta", "dbias", "running_mean", "running_var"), got, refs, errs):
        if r_ is None:
            assert g_ is None, n
        else:
            _check(n, g_, r_, e_, False)
    assert int(nbt) == (4 if train else 3)
    if not train and bn:
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)


# ====================================================================== the module
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "conv_mixer.npz"))


def _module(gold, case, compute_dtype, drop=0.0):
    from htrvt_amd.mixer import ConvLocalMixer1D
    use_bn = C.CASES[case][2]
    m = ConvLocalMixer1D(C.D, C.K, drop=drop, use_bn=use_bn, compute_dtype=compute_dtype)
    sd = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd.") and k[3:] in m.state_dict()}
    if not use_bn:
        sd["dwconv.bias"] = torch.from_numpy(gold["nobn.dwconv.bias"])
    m.load_state_dict(sd, strict=True)
    return m.cuda(), {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def _rel(name, got, ref, gate):
    ref = torch.as_tensor(ref, dtype=F64)
    err = float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"  {name}: {err:.2e} (gate {gate:.0e})")
    assert err < gate, (name, err)


@pytest.mark.parametrize("cdt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(C.CASES))
def test_module_reproduces_the_fork(gold, case, cdt):
    """outputs within 1e-3 of max |ref| and gradients within 2e-3 in float32 (the window model's gates); bfloat16 printed and
    gated at 5e-2 / 1e-1"""
    import htrvt_amd  # noqa: F401
    go, gg = (1e-3, 2e-3) if cdt == F32 else (5e-2, 1e-1)
    m, _ = _module(gold, case, cdt)
    x, dy = [t.cuda() for t in C.inputs(case)]
    print(f"\nConvLocalMixer1D {case} {cdt}")
    with pytest.raises(RuntimeError):
        m(x.cpu())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        y = m.eval()(x)
    _rel("y_eval", y, gold[case + ".y_eval"], go)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k               # eval mode leaves the buffers untouched
    xr = x.clone().requires_grad_(True)
    y = m.train()(xr)
    assert y.grad_fn is not None and y.grad_fn.name().startswith("_MixerFunction")
    y.backward(dy)
    _rel("y_train", y, gold[case + ".y_train"], go)
    _rel("dx", xr.grad, gold[case + ".dx"], gg)
    for n, p in m.named_parameters():
        _rel("grad " + n, p.grad, gold[f"{case}.grad.{n}"], gg)
    if C.CASES[case][2]:
        _rel("running_mean", m.bn.running_mean, gold[case + ".running_mean"], go)
        _rel("running_var", m.bn.running_var, gold[case + ".running_var"], go)
        assert int(m.bn.num_batches_tracked) == int(gold[case + ".num_batches_tracked"])


def test_module_dropout(gold):
    """p = 0.1 on (3, 33, 64): the same seed gives the same output; every element of y_p - x is 0 or (y_0 - x) / (1 - p);
    the dropped share is within 5 sigma of p (sigma = sqrt(p (1 - p) / 6336) = 0.0038); the gradients are those of the
    float64 reference run with the recovered mask"""
    import htrvt_amd  # noqa: F401
    case, p = "b3n33", 0.1
    m, sd64 = _module(gold, case, F32, drop=p)
    x, dy = [t.cuda() for t in C.inputs(case)]
    m.train()
    ys = []
    for _ in range(2):
        torch.cuda.manual_seed(77)
        m.zero_grad()
        xr = x.clone().requires_grad_(True)
        y = m(xr)
        y.backward(dy)
        ys.append(y.detach())
    assert torch.equal(ys[0], ys[1])
    grads = {n: q.grad.clone() for n, q in m.named_parameters()}
    dx = xr.grad.clone()
    m.drop.p = 0.0
    with torch.no_grad():
        y0 = m(x)
    m.drop.p = p
    o_p, o_0 = (ys[0] - x).double().cpu().view(-1, C.D), (y0 - x).double().cpu().view(-1, C.D) / (1 - p)
    # y and x are float32: a difference y - x carries up to two roundings of magnitude 2^-24 max|y|, the scaling one more
    tol = 16 * 2.0 ** -24 * float(y0.abs().max())
    kept = (o_p - o_0).abs() <= tol
    dropped = o_p == 0
    assert bool((kept | dropped).all())
    clear = o_0.abs() > 2 * tol                 # where "kept" and "dropped" cannot both hold
    share = float((dropped & clear).sum()) / float(clear.sum())
    print(f"\ndropout: dropped share {share:.4f} of {int(clear.sum())} elements")
    assert abs(share - p) <= 0.019
    keep = (~(dropped & clear)).double()
    dx_r, g_r = M.mixer_module_grads(sd64, x.double().cpu(), dy.double().cpu(), training=True, keep=keep, drop_p=p)
    _rel("dx", dx, dx_r, 2e-3)
    for n, g_ in grads.items():
        _rel("grad " + n, g_, g_r[n], 2e-3)
