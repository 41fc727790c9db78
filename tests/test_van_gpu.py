"""The VAN forks' operators on the MI355X: csrc/van.hip through the C ABI against tests/van_refs.py in float64, the autograd
wrapper variants.depthwise_conv2d, and htrvt_amd.van.VANHeightReducer / HorizontalMixer against tests/golden/van.npz (the
fork's own modules in float64).

Kernel gates follow tests/test_conv_mixer_gpu.py: per element against the float64 reference over the same (already
rounded) inputs, relative to the reference's largest magnitude, gate = 8 * E32 (+ 2^-8 |ref| for a bfloat16 output) with
E32 = kernel_refs.e32, the float32 evaluation error of the reference itself on these inputs.  Nothing in a gate comes from
the kernel under test.  Every output buffer carries one canary row behind it that must stay untouched.  Every comparison
prints E32, gate and observed error (`pytest -s`).

Module gates are ConvLocalMixer1D's, relative to the largest reference magnitude per tensor: float32 outputs and buffers
1e-3, gradients 2e-3; bfloat16 5e-2 and 1e-1.  One tensor has no magnitude of its own: proj2.bias feeds a train-mode
BatchNorm, which removes it, so its gradient is a sum that cancels to rounding noise (1e-17 in the fixture); its error is
taken relative to the largest per-channel sum of the magnitudes of that sum's terms, which the fixture records.

Measured on an MI355X, over all parametrised cases of an output (errors relative to max |ref|; a bfloat16 gate is
2^-8 = 3.9e-3 plus 8 * E32):

  output                            E32 (range)        worst observed   worst observed / gate
  depthwise y              bf16     2.7e-8 .. 2.5e-7   3.4e-3           0.86
  depthwise y              f32      1.5e-8 .. 2.0e-7   1.8e-7           0.15
  depthwise dx, dx + add   bf16     2.8e-8 .. 2.5e-7   3.2e-3           0.81
  depthwise dx, dx + add   f32      4.8e-8 .. 2.5e-7   2.2e-7           0.17
  depthwise dw                      0 .. 1.4e-7        2.1e-7           0.20
  gate g / da / dz         bf16     0 .. 9.9e-8        2.6e-3           0.66     (dz = dg * a is exact in float32: E32 = 0)
  gate g / da / dz         f32      1.7e-8 .. 9.4e-8   8.6e-8           0.13
  bn_res_gelu y / dt       bf16     3.3e-8 .. 1.2e-7   3.5e-3           0.88
  bn_res_gelu y / dt       f32      3.4e-8 .. 1.3e-7   1.2e-7           0.18
  pool, pool dx            bf16     0 .. 3.3e-8        2.6e-3           0.67
  pool, pool dx            f32      0 .. 8.6e-8        9.2e-8           0.25
  moments                           1.2e-10 .. 1.4e-7  1.1e-7           0.21
  variants wrapper, f32: y, dx, dw  5.1e-8 .. 1.5e-7   1.5e-7           0.15
  VANHeightReducer, float32: outputs 3.5e-7, buffers 9.7e-8 (gate 1e-3), gradients 9.0e-7 (gate 2e-3)
  VANHeightReducer, bfloat16: outputs 9.7e-3, buffers 3.0e-4 (gate 5e-2), gradients 2.2e-2 (gate 1e-1)
  HorizontalMixer, float32: outputs 2.6e-7, buffers 1.0e-7 (gate 1e-3), gradients 3.5e-7 (gate 2e-3)
  HorizontalMixer, bfloat16: outputs 4.2e-3, buffers 2.3e-4 (gate 5e-2), gradients 6.1e-3 (gate 1e-1)
  VANHeightReducer on (2, 32, 4, 1024), split weight gradients: float32 output 3.5e-7, gradients 1.2e-6; bfloat16 output
  8.7e-3, gradients 1.9e-2; proj2.bias against the sum of |terms| 6.8e-9 / 5.8e-5

Per-launch times (tools/bench_van.py, B = 128, W = 128, C = 768, bfloat16; share of the launch's HBM floor, the tensor
bytes read once and written once at 6.3 TB/s): 5x5 d1 at H = 4 forward 152 us (0.21), input gradient 149 us (0.21), weight
gradient 150 us (0.24); 7x7 d3 at H = 4 forward 83 us (0.38), input gradient 84 us (0.38), weight gradient 140 us (0.26);
1x9 d1 at H = 1 forward 25.8 us (0.31), input gradient 26.0 us (0.31), weight gradient 54 us (0.17).  DESIGN 4k says what
bounds them.
"""
import os

import numpy as np
import pytest
import torch

import kernel_refs as R
import van_cases as C
import van_refs as V

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import colsum, dt, ptr, stream
    return lib, check, ptr, stream, dt, colsum


def _check(name, got, ref, err, bf16_out):
    ok, obs = R.gate_check(name, got.detach().cpu(), ref, err, bf16_out)
    assert ok, f"{name}: observed {obs:.3e} of max|ref| is outside 8 * E32 = {8 * err:.3e}" + (" + one bf16 ulp" if bf16_out else "")


def _out(shape, dtype):
    """an output buffer of `shape` with one canary row (the last dimension) behind it -> (whole buffer, the output's view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + shape[-1],), 7.0, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


def _intact(*bufs_and_shapes):
    for buf, view in bufs_and_shapes:
        assert (buf[view.numel():] == 7).all(), "the canary row behind an output was written"


# ====================================================================== depthwise convolution
@DTYPES
@pytest.mark.parametrize("shape", C.DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depthwise_kernels_against_float64(shape, dtype):
    lib, check, ptr, stream, dt, colsum = _lib()
    B, H, W, Cc, kh, kw, dil = shape
    geo = (B, H, W, Cc, kh, kw, dil, dt(dtype))
    bf = dtype == BF
    x, dy, w = C.dw_inputs(shape, dtype)
    print(f"\ndepthwise {dtype} {shape}")
    xd, dyd, wd = x.cuda(), dy.cuda(), w.cuda()
    y = _out(x.shape, dtype)
    check(lib.htrvt_van_dw_fwd(ptr(xd), ptr(wd), ptr(y[1]), *geo, stream()), "dw_fwd")
    (y_r,), (e,) = R.e32(lambda a, b: V.dwconv(a, b, kh, kw, dil), [x.float(), w])
    _check("y", y[1].float(), y_r, e, bf)

    dx, dxa = _out(x.shape, dtype), _out(x.shape, dtype)
    check(lib.htrvt_van_dw_bwd_input(ptr(dyd), ptr(wd), None, ptr(dx[1]), *geo, stream()), "dw_bwd_input")
    check(lib.htrvt_van_dw_bwd_input(ptr(dyd), ptr(wd), ptr(xd), ptr(dxa[1]), *geo, stream()), "dw_bwd_input + add")
    (dx_r, dxa_r), (e1, e2) = R.e32(lambda g, b, a: (V.dwconv_bwd_input(g, b, kh, kw, dil), V.dwconv_bwd_input(g, b, kh, kw, dil, add=a)),
                                    [dy.float(), w, x.float()])
    _check("dx", dx[1].float(), dx_r, e1, bf)
    _check("dx + add", dxa[1].float(), dxa_r, e2, bf)

    rows = lib.htrvt_van_dw_rows(*geo)
    assert rows >= H and rows % H == 0 and lib.htrvt_van_dw_bwd_workspace_floats(*geo) == rows * Cc * kh * kw
    part = _out((rows, Cc * kh * kw), F32)
    check(lib.htrvt_van_dw_bwd_weight(ptr(xd), ptr(dyd), ptr(part[1]), *geo, stream()), "dw_bwd_weight")
    dw = torch.zeros(Cc, kh * kw, device="cuda")
    colsum(part[1], rows, Cc * kh * kw, Cc * kh * kw, dw, dti=0)
    (dw_r,), (e,) = R.e32(lambda a, g: V.dwconv_bwd_weight(a, g, kh, kw, dil), [x.float(), dy.float()])
    _check("dw", dw, dw_r, e, False)
    _intact(y, dx, dxa, part)


@DTYPES
@pytest.mark.parametrize("shape", [(2, 4, 7, 8, 7, 7, 3), (2, 4, 33, 24, 5, 5, 1), (3, 1, 130, 64, 1, 9, 1)], ids=lambda s: "x".join(map(str, s)))
def test_exact_case_and_images_do_not_see_each_other(shape, dtype):
    """integers -2 ... 2 and taps from {+-0.5, +-1, +-2}: at most 20 live taps, so every partial sum is a multiple of 0.5
    below 128 and representable in bfloat16, and y and dx equal the reference bit for bit; and changing every image but
    the first leaves the first image's results bit for bit"""
    lib, check, ptr, stream, dt, _ = _lib()
    B, H, W, Cc, kh, kw, dil = shape
    geo = (B, H, W, Cc, kh, kw, dil, dt(dtype))
    g = torch.Generator().manual_seed(W + kw)
    x = torch.randint(-2, 3, (B, H, W, Cc), generator=g).float()
    w = torch.tensor((-2.0, -1.0, -0.5, 0.5, 1.0, 2.0))[torch.randint(0, 6, (Cc, kh * kw), generator=g)]
    y_r, dx_r = V.dwconv(x.double(), w.double(), kh, kw, dil), V.dwconv_bwd_input(x.double(), w.double(), kh, kw, dil)
    assert torch.equal(y_r.to(dtype).double(), y_r) and torch.equal(dx_r.to(dtype).double(), dx_r)
    x2 = x.clone()
    x2[1:] = x2[1:] * -3 + 1
    outs = []
    for xx in (x, x2):
        xd, wd = xx.to(dtype).cuda(), w.cuda()
        y, dx = torch.empty_like(xd), torch.empty_like(xd)
        check(lib.htrvt_van_dw_fwd(ptr(xd), ptr(wd), ptr(y), *geo, stream()), "dw_fwd")
        check(lib.htrvt_van_dw_bwd_input(ptr(xd), ptr(wd), None, ptr(dx), *geo, stream()), "dw_bwd_input")
        rows = lib.htrvt_van_dw_rows(1, *geo[1:])
        part = torch.empty(rows, Cc * kh * kw, device="cuda")      # the first image alone: its weight gradient
        check(lib.htrvt_van_dw_bwd_weight(ptr(xd), ptr(xd), ptr(part), 1, *geo[1:], stream()), "dw_bwd_weight")
        outs.append((y, dx, part))
    assert torch.equal(outs[0][0].double().cpu(), y_r) and torch.equal(outs[0][1].double().cpu(), dx_r)
    for a, b in zip(*outs):
        assert torch.equal(a[:1], b[:1]) if a.dim() == 4 else torch.equal(a, b)
        assert a.dim() != 4 or not torch.equal(a[1:], b[1:])


# ====================================================================== gate, BatchNorm + shortcut + GELU, pool, moments
@DTYPES
@pytest.mark.parametrize("shape", C.EW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_elementwise_and_pool_kernels_against_float64(shape, dtype):
    lib, check, ptr, stream, dt, _ = _lib()
    B, H, W, Cc = shape
    rows, dti, bf = B * H * W, dt(dtype), dtype == BF
    (a, p, dg, res), scale, shift = C.ew_inputs(shape, dtype)
    print(f"\nelement-wise {dtype} {shape}")
    ad, pd, dgd, resd, scd, shd = [t.cuda() for t in (a, p, dg, res, scale, shift)]
    flat = lambda t: t.float().reshape(rows, Cc)                              # noqa: E731

    g = _out(a.shape, dtype)
    check(lib.htrvt_van_gate_fwd(ptr(ad), ptr(pd), ptr(scd), ptr(shd), ptr(g[1]), rows, Cc, dti, stream()), "gate_fwd")
    (g_r,), (e,) = R.e32(V.gate_fwd, [flat(a), flat(p), scale, shift])
    _check("gate g", g[1].float().view(rows, Cc), g_r, e, bf)
    da, dz = _out(a.shape, dtype), _out(a.shape, dtype)
    check(lib.htrvt_van_gate_bwd(ptr(dgd), ptr(ad), ptr(pd), ptr(scd), ptr(shd), ptr(da[1]), ptr(dz[1]), rows, Cc, dti, stream()),
          "gate_bwd")
    (da_r, dz_r), (e1, e2) = R.e32(V.gate_bwd, [flat(dg), flat(a), flat(p), scale, shift])
    _check("gate da", da[1].float().view(rows, Cc), da_r, e1, bf)
    _check("gate dz", dz[1].float().view(rows, Cc), dz_r, e2, bf)

    for with_res in (True, False):
        r_h, r_d = (flat(res), ptr(resd)) if with_res else (None, None)
        sc_h, sh_h, sc_d, sh_d = (scale, shift, ptr(scd), ptr(shd)) if with_res else (None, None, None, None)
        y, dt_ = _out(a.shape, dtype), _out(a.shape, dtype)
        check(lib.htrvt_van_bn_res_gelu_fwd(ptr(pd), sc_d, sh_d, r_d, ptr(y[1]), rows, Cc, dti, stream()), "bn_res_gelu_fwd")
        check(lib.htrvt_van_bn_res_gelu_bwd(ptr(dgd), ptr(pd), sc_d, sh_d, r_d, ptr(dt_[1]), rows, Cc, dti, stream()),
              "bn_res_gelu_bwd")
        (y_r, dt_r), (e1, e2) = R.e32(lambda x_, s_, h_, r_, d_: (V.bn_res_gelu_fwd(x_, s_, h_, r_), V.bn_res_gelu_bwd(d_, x_, s_, h_, r_)),
                                      [flat(p), sc_h, sh_h, r_h, flat(dg)])
        tag = "" if with_res else " (plain gelu)"
        _check("bn_res_gelu y" + tag, y[1].float().view(rows, Cc), y_r, e1, bf)
        _check("bn_res_gelu dt" + tag, dt_[1].float().view(rows, Cc), dt_r, e2, bf)
        _intact(y, dt_)

    pool, dpool = _out((B, W, Cc), dtype), _out(a.shape, dtype)
    check(lib.htrvt_van_hpool_fwd(ptr(ad), ptr(pool[1]), B, H, W, Cc, dti, stream()), "hpool_fwd")
    d = dg[:, 0].contiguous()
    dd = d.cuda()
    check(lib.htrvt_van_hpool_bwd(ptr(dd), ptr(dpool[1]), B, H, W, Cc, dti, stream()), "hpool_bwd")
    (pool_r, dpool_r), (e1, e2) = R.e32(lambda x_, d_: (V.hpool_fwd(x_), V.hpool_bwd(d_, H)), [a.float(), d.float()])
    _check("pool", pool[1].float(), pool_r, e1, bf)
    _check("pool dx", dpool[1].float(), dpool_r, e2, bf)

    Q = lib.htrvt_van_moments_rows(rows, Cc, dti)
    assert 1 <= Q <= 128
    part = _out((Q, 2, Cc), F32)
    check(lib.htrvt_van_moments(ptr(ad), ptr(part[1]), rows, Cc, dti, stream()), "moments")
    (m_r,), (e,) = R.e32(V.moments, [flat(a)])
    _check("moments", part[1].double().sum(0, keepdim=True), m_r, e, False)
    _intact(g, da, dz, pool, dpool, part)


def test_refusals_launch_nothing():
    lib, check, ptr, stream, dt, _ = _lib()
    B, H, W, Cc = 2, 3, 6, 16
    for dtype in (BF, F32):
        dti = dt(dtype)
        x = torch.ones(B * H * W + 1, Cc, dtype=dtype, device="cuda")
        out = torch.full((B * H * W + 1, Cc), 7.0, dtype=dtype, device="cuda")
        out2 = torch.full((B * H * W + 1, Cc), 7.0, dtype=dtype, device="cuda")
        w = torch.ones(Cc, 81, device="cuda")
        ws = torch.full((65536,), 7.0, device="cuda")
        vec = torch.ones(Cc, device="cuda")
        off = 4 if dtype == F32 else 2      # one element: no longer 16-byte aligned
        st = stream()

        def conv(xp, op, c, kh, kw, dil, wp=ptr(w), weight_too=True):
            rcs = (lib.htrvt_van_dw_fwd(xp, wp, op, B, H, W, c, kh, kw, dil, dti, st),
                   lib.htrvt_van_dw_bwd_input(xp, wp, None, op, B, H, W, c, kh, kw, dil, dti, st))
            if weight_too:
                rcs += (lib.htrvt_van_dw_bwd_weight(xp, xp, None if op is None else ptr(ws), B, H, W, c, kh, kw, dil, dti, st),)
            return rcs
        bad = {"even kh": conv(ptr(x), ptr(out), Cc, 4, 5, 1), "even kw": conv(ptr(x), ptr(out), Cc, 5, 4, 1),
               "kh = 9": conv(ptr(x), ptr(out), Cc, 9, 5, 1), "kw = 11": conv(ptr(x), ptr(out), Cc, 5, 11, 1),
               "kh = 0": conv(ptr(x), ptr(out), Cc, 0, 5, 1), "dil = 0": conv(ptr(x), ptr(out), Cc, 5, 5, 0),
               "dil = 4": conv(ptr(x), ptr(out), Cc, 5, 5, 4), "C = 12": conv(ptr(x), ptr(out), 12, 5, 5, 1),
               "x unaligned": conv(ptr(x) + off, ptr(out), Cc, 5, 5, 1), "null x": conv(None, ptr(out), Cc, 5, 5, 1),
               "null w": conv(ptr(x), ptr(out), Cc, 5, 5, 1, wp=None, weight_too=False), "null out": conv(ptr(x), None, Cc, 5, 5, 1),
               "out unaligned": conv(ptr(x), ptr(out) + off, Cc, 5, 5, 1, weight_too=False),
               "add unaligned": (lib.htrvt_van_dw_bwd_input(ptr(x), ptr(w), ptr(x) + off, ptr(out), B, H, W, Cc, 5, 5, 1, dti, st),)}
        n = B * H * W

        def ew(ap, op, c, moments_too=True):
            rcs = (lib.htrvt_van_gate_fwd(ap, ap, ptr(vec), ptr(vec), op, n, c, dti, st),
                    lib.htrvt_van_gate_bwd(ap, ap, ap, ptr(vec), ptr(vec), op, None if op is None else ptr(out2), n, c, dti, st),
                    lib.htrvt_van_bn_res_gelu_fwd(ap, ptr(vec), ptr(vec), None, op, n, c, dti, st),
                    lib.htrvt_van_bn_res_gelu_bwd(ap, ap, ptr(vec), ptr(vec), None, op, n, c, dti, st),
                    lib.htrvt_van_hpool_fwd(ap, op, B, H, W, c, dti, st), lib.htrvt_van_hpool_bwd(ap, op, B, H, W, c, dti, st))
            if moments_too:
                rcs += (lib.htrvt_van_moments(ap, None if op is None else ptr(ws), n, c, dti, st),)
            return rcs
        bad.update({"ew C = 12": ew(ptr(x), ptr(out), 12), "ew in unaligned": ew(ptr(x) + off, ptr(out), Cc),
                    "ew out unaligned": ew(ptr(x), ptr(out) + off, Cc, moments_too=False), "ew null in": ew(None, ptr(out), Cc),
                    "ew null out": ew(ptr(x), None, Cc),
                    "gate dz unaligned": (lib.htrvt_van_gate_bwd(ptr(x), ptr(x), ptr(x), ptr(vec), ptr(vec), ptr(out), ptr(out2) + off, n,
                                                                 Cc, dti, st),),
                    "res unaligned": (lib.htrvt_van_bn_res_gelu_fwd(ptr(x), ptr(vec), ptr(vec), ptr(x) + off, ptr(out), n, Cc, dti, st),)})
        for what, rcs in bad.items():
            assert all(rc < 0 for rc in rcs), (what, rcs)
        assert lib.htrvt_last_error()
        torch.cuda.synchronize()
        assert (out == 7).all() and (out2 == 7).all() and (ws == 7).all()
        assert lib.htrvt_van_dw_rows(B, H, W, 12, 5, 5, 1, dti) < 0 and lib.htrvt_van_dw_bwd_workspace_floats(B, H, W, Cc, 4, 5, 1, dti) < 0
        assert lib.htrvt_van_moments_rows(n, 12, dti) < 0


# ====================================================================== the autograd wrapper, reproducibility
@pytest.mark.parametrize("shape", [(2, 4, 7, 8, 7, 7, 3), (2, 4, 33, 24, 5, 5, 1), (3, 1, 130, 64, 1, 9, 1)], ids=lambda s: "x".join(map(str, s)))
def test_variants_depthwise_conv2d_against_float64_autograd(shape):
    """variants.depthwise_conv2d in float32 against autograd through torch's own float64 conv2d; gates from the float32
    evaluation of the same, as above"""
    import htrvt_amd  # noqa: F401
    import torch.nn.functional as F
    from htrvt_amd import variants
    B, H, W, Cc, kh, kw, dil = shape
    x, dy, w = C.dw_inputs(shape, F32, seed=1)
    print(f"\ndepthwise_conv2d {shape}")

    def ref(x_, w_, dy_):
        xr, wr = x_.permute(0, 3, 1, 2).clone().requires_grad_(True), w_.reshape(Cc, 1, kh, kw).clone().requires_grad_(True)
        y_ = F.conv2d(xr, wr, padding=((kh // 2) * dil, (kw // 2) * dil), dilation=dil, groups=Cc)
        (y_ * dy_.permute(0, 3, 1, 2)).sum().backward()
        return y_.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad
    refs, errs = R.e32(ref, [x, w, dy])
    xd, wd = x.cuda().requires_grad_(True), w.view(Cc, 1, kh, kw).cuda().requires_grad_(True)
    y = variants.depthwise_conv2d(xd, wd, dilation=dil)
    assert y.grad_fn is not None and y.grad_fn.name().startswith("_DepthwiseConv2d")
    y.backward(dy.cuda())
    for n, g_, r_, e_ in zip(("y", "dx", "dw"), (y, xd.grad, wd.grad), refs, errs):
        _check(n, g_, r_, e_, False)
    with pytest.raises(RuntimeError):
        variants.depthwise_conv2d(x, w.view(Cc, 1, kh, kw))
    with pytest.raises(TypeError):
        variants.depthwise_conv2d(xd, wd.detach().bfloat16())


@DTYPES
def test_backward_twice_gives_the_same_bits(dtype):
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    shape = (2, 4, 128, 768, 7, 7, 3)
    x, dy, w = [t.cuda() for t in C.dw_inputs(shape, dtype, seed=2)]
    w = w.view(768, 1, 7, 7).contiguous()
    runs = [seq_ops.dwconv_bwd(dy, x, w, 3) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ====================================================================== the modules
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "van.npz"))


def _module(gold, tag, compute_dtype):
    from htrvt_amd import van
    if tag == "red":
        m, prefix = van.VANHeightReducer(C.D, depth=C.DEPTH, compute_dtype=compute_dtype), "sd.van_reducer."
    else:
        m, prefix = van.HorizontalMixer(C.D, k=C.K, compute_dtype=compute_dtype), "sd.hmix."
    m.load_state_dict({k[len(prefix):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(prefix)}, strict=True)
    return m.cuda()


def _rel(name, got, ref, gate, scale=None):
    ref = torch.as_tensor(ref, dtype=F64)
    err = float((got.detach().double().cpu() - ref).abs().max() / (ref.abs().max() if scale is None else scale))
    print(f"  {name}: {err:.2e} (gate {gate:.0e})")
    assert err < gate, (name, err)


@pytest.mark.parametrize("cdt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("tag", ["red", "mix"])
@pytest.mark.parametrize("case", list(C.CASES))
def test_modules_reproduce_the_fork(gold, case, tag, cdt):
    import htrvt_amd  # noqa: F401
    go, gg = (1e-3, 2e-3) if cdt == F32 else (5e-2, 1e-1)
    m = _module(gold, tag, cdt)
    ins = C.inputs(case)
    x, dy = [t.cuda() for t in (ins[:2] if tag == "red" else ins[2:])]
    pre = f"{case}.{tag}."
    print(f"\n{type(m).__name__} {case} {cdt}")
    with pytest.raises(RuntimeError):
        m(x.cpu())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        y = m.eval()(x)
    assert y.dtype == F32 and tuple(y.shape) == tuple(dy.shape)
    _rel("y_eval", y, gold[pre + "y_eval"], go)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k               # eval mode leaves the buffers untouched
    with torch.no_grad():                                 # any memory format of the input: the same bits
        assert torch.equal(m(x.contiguous(memory_format=torch.channels_last)), y)
    xr = x.clone().requires_grad_(True)
    y = m.train()(xr)
    nodes, fn = [], y.grad_fn
    while fn is not None:                                 # the chain of nodes from the output back to the input
        nodes.append(fn.name())
        inner = [f for f, _ in fn.next_functions if f is not None and "AccumulateGrad" not in f.name()]
        fn = inner[0] if inner else None
    want = ["_PoolFunction"] + ["_BlockFunction"] * C.DEPTH + ["_ToNHWC"] if tag == "red" else ["_MixerFunction"]
    assert [n.replace("Backward", "") for n in nodes[:len(want)]] == want, nodes
    y.backward(dy)
    _rel("y_train", y, gold[pre + "y_train"], go)
    _rel("dx", xr.grad, gold[pre + "dx"], gg)
    for n, p in m.named_parameters():
        key = f"{pre}gradscale.{n}"
        _rel("grad " + n, p.grad, gold[f"{pre}grad.{n}"], gg, float(gold[key]) if key in gold.files else None)
    for n, b in m.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(gold[pre + "buf." + n])
        else:
            _rel(n, b, gold[pre + "buf." + n], go)


@pytest.mark.parametrize("cdt", [F32, BF], ids=["f32", "bf16"])
def test_wide_map_takes_the_split_weight_gradients(gold, cdt):
    """(2, 32, 4, 1024): 8192 rows, where the 1x1 weight gradients are contracted in four ranges (seq_ops.wgrad_split_k)
    and the statistics and depthwise passes run past one workgroup of rows; against the float64 statement of the reducer on
    the same inputs, at the module gates, and twice for the same bits"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    B, H, W = 2, 4, 1024
    assert seq_ops.wgrad_split_k(B * H * W, C.D, C.D) == 4 and seq_ops.wgrad_split_k(2047, C.D, C.D) == 1
    assert seq_ops.wgrad_split_k(128 * 4 * 128, 768, 768) == 16
    go, gg = (1e-3, 2e-3) if cdt == F32 else (5e-2, 1e-1)
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(B, C.D, H, W, generator=g), torch.randn(B, C.D, 1, W, generator=g)
    sd = {k[len("sd.van_reducer."):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd.van_reducer.")}
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    taps = {}
    fn = lambda s_, t_: V.reducer(s_, t_, True, C.DEPTH, taps=taps)          # noqa: E731
    y_r = fn(sd64, x.double())[0].detach()
    dx_r, g_r = V.module_grads(fn, sd64, x.double(), dy.double())
    runs = []
    for _ in range(2):
        m = _module(gold, "red", cdt).train()
        xr = x.cuda().requires_grad_(True)
        y = m(xr)
        y.backward(dy.cuda())
        runs.append([y.detach(), xr.grad] + [p.grad for p in m.parameters()])
    for a_, b_ in zip(*runs):
        assert torch.equal(a_, b_)
    print(f"\nVANHeightReducer (2, {C.D}, 4, 1024) {cdt}")
    _rel("y_train", y, y_r, go)
    _rel("dx", xr.grad, dx_r, gg)
    for n, p in m.named_parameters():
        # proj2.bias: a sum that cancels (see the module docstring); measured against the largest sum of |terms|
        scale = float(taps[n].grad.abs().sum(0).max()) if n in taps else None
        _rel("grad " + n, p.grad, g_r[n], gg, scale)


def test_blocks_on_their_own(gold):
    """a VANBlock called on its own is the reducer's block (the reducer of depth 1 is its mean over the height), a
    LargeKernelAttention on its own reproduces the float64 statement of it, and drop_path > 0 is refused in train mode only"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import van
    torch.manual_seed(3)
    red = C.perturb(van.VANHeightReducer(16, depth=1)).cuda().eval()
    x = torch.randn(2, 16, 4, 9, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        y_blk = red.blocks[0](x.cuda())
        assert tuple(y_blk.shape) == tuple(x.shape) and y_blk.dtype == F32
        _rel("reducer of one block", red(x.cuda()), y_blk.double().mean(2, keepdim=True).cpu(), 1e-6)
        g = red.blocks[0].lka(x.cuda())
    sd = {k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in red.blocks[0].lka.state_dict().items()}
    g_r = V.lka(x.double().permute(0, 2, 3, 1), sd, "", False, {}).reshape(2, 4, 9, 16).permute(0, 3, 1, 2)
    _rel("LargeKernelAttention", g, g_r, 1e-3)
    blk = van.VANBlock(16, drop_path=0.1).cuda()
    with torch.no_grad():
        blk.eval()(x.cuda())
    with pytest.raises(NotImplementedError):
        blk.train()(x.cuda())
