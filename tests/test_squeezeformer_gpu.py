"""The convolutional forks' blocks on the MI355X: csrc/gnmixer.hip through the C ABI against tests/squeezeformer_refs.py in
float64, the autograd operators of htrvt_amd.variants, and the modules of htrvt_amd.conformer against squeezeformer_refs
over the state_dicts of tests/golden/squeezeformer.npz (tests/test_squeezeformer_cpu.py ties squeezeformer_refs to the
fork's own modules at 1e-10).

Kernel gates follow tests/test_conv_mixer_gpu.py: per element against the float64 reference over the same (already rounded)
inputs, relative to the reference's largest magnitude, gate = 8 * E32 (+ 2^-8 |ref| for a bfloat16 output) with
E32 = kernel_refs.e32, the float32 evaluation error of the reference itself on these inputs.  Nothing in a gate comes from
the kernel under test.  The launches are checked stage by stage, a later stage's reference taking the earlier launches'
outputs as its inputs (c as stored, the statistics), as the kernels do.  Output buffers carry canaries past their ends.
The backward's per-image sums (sum gamma dz, sum gamma dz xhat) are judged as the [B][2] tensor the kernel writes: each is a
sum of C * N signed terms that cancels to a hundredth of their magnitudes, so the float32 error of any evaluation of ONE such
number is a draw between 0 and a few 1e-7 (E32 of a single image's sum ranged from 6e-9 to 6e-7 over the cases), and a
gate taken from two draws can be ten times below the float32 rounding of the terms themselves; over the 2 B values it is
a stable figure.  htrvt_gn_bwd_finalize is checked bit for bit against the same ordered float64 sum.
Module gates are the project's: relative to the tensor's maximum, float32 1e-3 (outputs) / 2e-3 (gradients), bfloat16
5e-2 / 1e-1.  Every comparison prints E32, gate and observed error (`pytest -s`).

Measured on an MI355X, worst over all parametrised cases of an output (errors relative to max |ref|; a bfloat16 gate is
2^-8 = 3.9e-3 plus 8 * E32):

  output                                   E32 (range)        worst observed    worst observed / gate
  mixer c, s, du               bf16        2.6e-8 .. 2.7e-7   2.7e-3            0.68
  mixer c, s, du               f32         2.8e-8 .. 2.9e-7   2.9e-7            0.24
  mixer mean / rstd                        0 .. 1.4e-7        8.4e-8 / 5.5e-8   0.16 / 0.22
  sum dz / sum dz xhat per channel         1.2e-8 .. 3.0e-7   2.0e-7 / 1.8e-7   0.22 / 0.43
  per-image pair [B][2]                    2.5e-8 .. 2.1e-7   2.3e-7            0.38
  m1, m2                                   bit-equal to the ordered float64 sum
  dw / dbias                               7.0e-8 .. 2.9e-7   2.2e-7 / 1.7e-7   0.19 / 0.24
  SE mean, pre, act, g, dg, dh2, dh1, dmean, dW, db   0 .. 6.4e-7   2.3e-7      0.37
  SE y, dx                     bf16 / f32  2.2e-8 .. 8.6e-8   3.2e-3 / 4.3e-8   0.81 / 0.13
  resampling                   bf16 / f32  0 .. 5.1e-8        3.3e-3 / 5.1e-8   0.84 / 0.13
  silu, silu bwd               bf16 / f32  5.6e-8 .. 2.9e-7   2.5e-3 / 1.5e-7   0.64 / 0.12
  operators, f32 (all outputs and gradients)   3.4e-8 .. 2.2e-7   2.3e-7        0.39
  modules, float32: outputs 1.5e-6 (gate 1e-3), gradients 3.1e-6 (gate 2e-3)
  modules, bfloat16: outputs 1.8e-2 (gate 5e-2), gradients 2.8e-2 (gate 1e-1)
  dropout p = 0.1: dropped share 0.0990 of 6336 unambiguous elements; gradients with the recovered mask 3.6e-7
"""
import os

import numpy as np
import pytest
import torch

import kernel_refs as R
import squeezeformer_cases as C
import squeezeformer_refs as S

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
EPS = float(torch.tensor(1e-5, dtype=F32))
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])


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


# ====================================================================== the GroupNorm mixer's launches, stage by stage
@DTYPES
@pytest.mark.parametrize("B,N,Cc,k", C.MIXER_SHAPES)
def test_gn_mixer_kernels_against_float64(B, N, Cc, k, dtype):
    lib, check, ptr, stream, dt, colsum = _lib()
    bf, dti, rows, cnt = dtype == BF, dt(dtype), B * N, float(Cc * N)
    u, ds, w, bias, gamma, beta = C.mixer_inputs(B, N, Cc, k, dtype)
    print(f"\ngn mixer {dtype} B={B} N={N} C={Cc} k={k}")
    d = {n: t.cuda() for n, t in dict(u=u, ds=ds, w=w, bias=bias, gamma=gamma, beta=beta).items()}
    P_, R_ = lib.htrvt_gnmixer_parts(B, N, Cc, dti), lib.htrvt_gnmixer_rows(B, N, Cc, dti)
    assert P_ >= 1 and R_ >= B and R_ % B == 0

    # ---- forward
    c, s = _canary(rows, Cc, dtype=dtype), _canary(rows, Cc, dtype=dtype)
    pairs, mean, rstd = _canary(B * P_, 2), _canary(B), _canary(B)
    check(lib.htrvt_gnmixer_fwd(ptr(d["u"]), ptr(d["w"]), ptr(d["bias"]), ptr(c), ptr(pairs), B, N, Cc, k, dti, stream()), "fwd")
    check(lib.htrvt_gn_finalize(ptr(pairs), B, P_, cnt, EPS, ptr(mean), ptr(rstd), stream()), "gn_finalize")
    check(lib.htrvt_gnmixer_act(ptr(c), ptr(mean), ptr(rstd), ptr(d["gamma"]), ptr(d["beta"]), ptr(s), B, N, Cc, dti, stream()), "act")
    (c_r,), (ec,) = R.e32(lambda a, b_, e: S.gn_conv(a, b_, e, B, N), [u.float(), w, bias])
    _check("c", c[:rows].float(), c_r, ec, bf)
    ck = c[:rows].float().cpu()
    (mean_r, rstd_r), (em, er) = R.e32(lambda a: S.gn_stats(a, B, N, EPS), [ck])
    _check("mean", mean[:B], mean_r, em, False)
    _check("rstd", rstd[:B], rstd_r, er, False)
    mean_h, rstd_h = mean[:B].cpu(), rstd[:B].cpu()
    (s_r,), (es,) = R.e32(lambda a, m, r, g, b_: S.gn_act(a, m, r, g, b_, N), [ck, mean_h, rstd_h, gamma, beta])
    _check("s", s[:rows].float(), s_r, es, bf)
    _intact(c, s, pairs, mean, rstd)

    # ---- backward
    pc, pairs2, m1, m2 = _canary(R_, 2 * Cc), _canary(B * P_, 2), _canary(B), _canary(B)
    check(lib.htrvt_gnmixer_bwd_reduce(ptr(d["ds"]), ptr(c), ptr(mean), ptr(rstd), ptr(d["gamma"]), ptr(d["beta"]), ptr(pc),
                                       ptr(pairs2), B, N, Cc, dti, stream()), "bwd_reduce")
    def sums(*a):                       # per channel two vectors [C]; per image the pair as the kernel writes it, [B][2]
        s1, s2, p1, p2 = S.gn_bwd_sums(*a, B, N)
        return s1, s2, torch.stack([p1, p2], 1)
    refs, errs = R.e32(sums, [ds.float(), ck, mean_h, rstd_h, gamma, beta])
    chan = pc[:R_].double().sum(0).cpu()
    pairs_h = pairs2[:B * P_].view(B, P_, 2).cpu()
    for n, g_, r_, e_ in zip(("sum dz", "sum dz xhat", "image pairs"), (chan[:Cc], chan[Cc:], pairs_h.double().sum(1)), refs, errs):
        _check(n, g_, r_, e_, False)
    check(lib.htrvt_gn_bwd_finalize(ptr(pairs2), B, P_, cnt, ptr(m1), ptr(m2), stream()), "gn_bwd_finalize")
    acc = torch.zeros(B, 2, dtype=F64)
    for i in range(P_):                 # the pairs in order, in float64, one rounding to float32: bit for bit
        acc += pairs_h[:, i].double()
    assert torch.equal(m1[:B].cpu(), (acc[:, 0] / cnt).float()) and torch.equal(m2[:B].cpu(), (acc[:, 1] / cnt).float())
    du, pw, pb = _canary(rows, 2 * Cc, dtype=dtype), _canary(R_, Cc * k), _canary(R_, Cc)
    check(lib.htrvt_gnmixer_bwd(ptr(d["u"]), ptr(c), ptr(d["ds"]), ptr(d["w"]), ptr(mean), ptr(rstd), ptr(d["gamma"]),
                                ptr(d["beta"]), ptr(m1), ptr(m2), ptr(du), ptr(pw), ptr(pb), B, N, Cc, k, dti, stream()), "bwd")
    dw, db = torch.zeros(Cc, k, device="cuda"), torch.zeros(Cc, device="cuda")
    colsum(pw, R_, Cc * k, Cc * k, dw, dti=0)
    colsum(pb, R_, Cc, Cc, db, dti=0)
    (du_r, dw_r, db_r), (edu, edw, edb) = R.e32(
        lambda *a: S.gn_core_bwd(*a, B, N), [ds.float(), ck, u.float(), w, mean_h, rstd_h, gamma, beta, m1[:B].cpu(), m2[:B].cpu()])
    _check("du", du[:rows].float(), du_r, edu, bf)
    _check("dw", dw, dw_r, edw, False)
    _check("dbias", db, db_r, edb, False)
    _intact(pc, pairs2, m1, m2, du, pw, pb)


@DTYPES
def test_images_do_not_see_each_other(dtype):
    """changing image 1's u leaves image 0's c, statistics, s and du bit for bit"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    B, N, Cc, k = 2, 5, 8, 3
    u, ds, w, bias, gamma, beta = [t.cuda() for t in C.mixer_inputs(B, N, Cc, k, dtype)]
    w = w.view(Cc, 1, k).contiguous()
    u2 = u.clone()
    u2[N:] = (u2[N:].float() * -3 + 1).to(dtype)
    out = []
    for uu in (u, u2):
        s, saved = seq_ops.gn_mixer_fwd(uu, w, bias, gamma, beta, B, N, EPS)
        du = seq_ops.gn_mixer_bwd(ds, uu, w, gamma, beta, B, N, saved)[0]
        out.append((saved[0], s, du, saved[1].view(B, 1).expand(B, N).reshape(-1), saved[2].view(B, 1).expand(B, N).reshape(-1)))
    for a, b in zip(*out):
        assert torch.equal(a[:N], b[:N])
        assert not torch.equal(a[N:], b[N:])


# ====================================================================== squeeze-excite
@DTYPES
@pytest.mark.parametrize("B,N,D", C.SE_SHAPES)
def test_se_kernels_against_float64(B, N, D, dtype):
    lib, check, ptr, stream, dt, _ = _lib()
    bf, dti, rows, H = dtype == BF, dt(dtype), B * N, C.se_hidden(D)
    x, dy, w1, b1, w2, b2 = C.se_inputs(B, N, D, dtype)
    print(f"\nsqueeze-excite {dtype} B={B} N={N} D={D} hidden={H}")
    d = {n: t.cuda() for n, t in dict(x=x, dy=dy, w1=w1, b1=b1, w2=w2, b2=b2).items()}
    mean, pre, act, g, y = _canary(B, D), _canary(B, H), _canary(B, H), _canary(B, D), _canary(rows, D, dtype=dtype)
    check(lib.htrvt_se_mean(ptr(d["x"]), ptr(mean), B, N, D, dti, stream()), "se_mean")
    check(lib.htrvt_se_mlp_fwd(ptr(mean), ptr(d["w1"]), ptr(d["b1"]), ptr(d["w2"]), ptr(d["b2"]), ptr(pre), ptr(act), ptr(g), B, D, H,
                               stream()), "se_mlp_fwd")
    check(lib.htrvt_se_scale_fwd(ptr(d["x"]), ptr(g), ptr(y), B, N, D, dti, stream()), "se_scale_fwd")
    (mean_r,), (em,) = R.e32(lambda a: S.se_mean(a, B, N), [x.float()])
    _check("mean", mean[:B], mean_r, em, False)
    mean_h = mean[:B].cpu()
    refs, errs = R.e32(S.se_mlp, [mean_h, w1, b1, w2, b2])
    for n, g_, r_, e_ in zip(("pre", "act", "g"), (pre, act, g), refs, errs):
        _check(n, g_[:B], r_, e_, False)
    g_h, pre_h, act_h = g[:B].cpu(), pre[:B].cpu(), act[:B].cpu()
    (y_r,), (ey,) = R.e32(lambda a, b_: S.se_scale(a, b_, N), [x.float(), g_h])
    _check("y", y[:rows].float(), y_r, ey, bf)
    _intact(mean, pre, act, g, y)

    dg, dh2, dh1, dmean = _canary(B, D), _canary(B, D), _canary(B, H), _canary(B, D)
    check(lib.htrvt_se_scale_bwd_reduce(ptr(d["dy"]), ptr(d["x"]), ptr(dg), B, N, D, dti, stream()), "se_scale_bwd_reduce")
    (dg_r,), (edg,) = R.e32(lambda a, b_: S.se_dg(a, b_, B, N), [dy.float(), x.float()])
    _check("dg", dg[:B], dg_r, edg, False)
    check(lib.htrvt_se_mlp_bwd(ptr(dg), ptr(g), ptr(pre), ptr(d["w1"]), ptr(d["w2"]), ptr(dh2), ptr(dh1), ptr(dmean), B, D, H,
                               stream()), "se_mlp_bwd")
    refs, errs = R.e32(S.se_mlp_bwd, [dg[:B].cpu(), g_h, pre_h, w1, w2])
    for n, g_, r_, e_ in zip(("dh2", "dh1", "dmean"), (dh2, dh1, dmean), refs, errs):
        _check(n, g_[:B], r_, e_, False)
    dw2, db2, dw1, db1 = _canary(D, H), _canary(D), _canary(H, D), _canary(H)
    check(lib.htrvt_se_wgrad(ptr(dh2), ptr(act), ptr(dw2), ptr(db2), B, D, H, stream()), "se_wgrad fc2")
    check(lib.htrvt_se_wgrad(ptr(dh1), ptr(mean), ptr(dw1), ptr(db1), B, H, D, stream()), "se_wgrad fc1")
    for tag, gw, gb, a_, b_ in (("fc2", dw2, db2, dh2[:B].cpu(), act_h), ("fc1", dw1, db1, dh1[:B].cpu(), mean_h)):
        (w_r, b_r), (ew, eb) = R.e32(S.se_wgrad, [a_, b_])
        _check("dW " + tag, gw[:-1], w_r, ew, False)
        _check("db " + tag, gb[:-1], b_r, eb, False)
    dx = _canary(rows, D, dtype=dtype)
    check(lib.htrvt_se_scale_bwd(ptr(d["dy"]), ptr(g), ptr(dmean), ptr(dx), B, N, D, dti, stream()), "se_scale_bwd")
    (dx_r,), (edx,) = R.e32(lambda a, b_, m: S.se_dx(a, b_, m, N), [dy.float(), g_h, dmean[:B].cpu()])
    _check("dx", dx[:rows].float(), dx_r, edx, bf)
    _intact(dg, dh2, dh1, dmean, dw2, db2, dw1, db1, dx)


# ====================================================================== resampling and SiLU
@DTYPES
@pytest.mark.parametrize("D", C.RESAMPLE_D)
@pytest.mark.parametrize("N0", C.RESAMPLE_N0)
def test_resampling_kernels_against_float64(N0, D, dtype):
    lib, check, ptr, stream, dt, _ = _lib()
    B, n, bf, dti = C.RESAMPLE_B, N0 // 2, dtype == BF, dt(dtype)
    g = torch.Generator().manual_seed(N0 + D)
    x, skip = torch.randn(B * N0, D, generator=g).to(dtype), torch.randn(B * N0, D, generator=g).to(dtype)
    ys = torch.randn(B * n, D, generator=g).to(dtype)
    print(f"\nresampling {dtype} B={B} N0={N0} D={D}")
    xd, sd_, yd = x.cuda(), skip.cuda(), ys.cuda()
    y, dx = _canary(B * n, D, dtype=dtype), _canary(B * N0, D, dtype=dtype)
    out, dys = _canary(B * N0, D, dtype=dtype), _canary(B * n, D, dtype=dtype)
    check(lib.htrvt_seq_down2_fwd(ptr(xd), ptr(y), B, N0, D, dti, stream()), "down2_fwd")
    check(lib.htrvt_seq_down2_bwd(ptr(yd), ptr(dx), B, N0, D, dti, stream()), "down2_bwd")
    check(lib.htrvt_seq_up_add_fwd(ptr(yd), ptr(sd_), ptr(out), B, n, N0, D, dti, stream()), "up_add_fwd")
    check(lib.htrvt_seq_up_add_bwd(ptr(xd), ptr(dys), B, n, N0, D, dti, stream()), "up_add_bwd")
    (r_,), (e_,) = R.e32(lambda a: S.down2(a, B, N0), [x.float()])
    _check("down2", y[:-1].float(), r_, e_, bf)
    (r_,), (e_,) = R.e32(lambda d_, a: S.grads_of(lambda t: S.down2(t, B, N0), d_, a)[0], [ys.float(), x.float()])
    _check("down2 dx", dx[:-1].float(), r_, e_, bf)
    if N0 % 2:
        assert (dx[:-1].view(B, N0, D)[:, -1] == 0).all()           # the dropped token
    (r_,), (e_,) = R.e32(lambda a, b_: S.up_add(a, b_, B, n, N0), [ys.float(), skip.float()])
    _check("up_add", out[:-1].float(), r_, e_, bf)
    (r_,), (e_,) = R.e32(lambda d_, a, b_: S.grads_of(lambda t: S.up_add(t, b_, B, n, N0), d_, a)[0],
                         [x.float(), ys.float(), skip.float()])
    _check("up_add dy", dys[:-1].float(), r_, e_, bf)
    _intact(y, dx, out, dys)


@DTYPES
def test_silu_kernels_against_float64(dtype):
    lib, check, ptr, stream, dt, _ = _lib()
    g = torch.Generator().manual_seed(9)
    rows, D = 37, 24
    pre, da = (torch.randn(rows, D, generator=g) * 3).to(dtype), torch.randn(rows, D, generator=g).to(dtype)
    a, dpre = _canary(rows, D, dtype=dtype), _canary(rows, D, dtype=dtype)
    print(f"\nsilu {dtype}")
    pre_d, da_d = pre.cuda(), da.cuda()
    check(lib.htrvt_silu_fwd(ptr(pre_d), ptr(a), rows * D, dt(dtype), stream()), "silu_fwd")
    check(lib.htrvt_silu_bwd(ptr(da_d), ptr(pre_d), ptr(dpre), rows * D, dt(dtype), stream()), "silu_bwd")
    (r_,), (e_,) = R.e32(S.silu, [pre.float()])
    _check("silu", a[:-1].float(), r_, e_, dtype == BF)
    (r_,), (e_,) = R.e32(S.silu_bwd, [da.float(), pre.float()])
    _check("silu bwd", dpre[:-1].float(), r_, e_, dtype == BF)
    _intact(a, dpre)


def test_refusals_launch_nothing():
    lib, check, ptr, stream, dt, _ = _lib()
    B, N, D = 2, 6, 16
    for dtype in (BF, F32):
        dti, off = dt(dtype), (4 if dtype == F32 else 2)      # one element: no longer 16-byte aligned
        bad_d = 12 if dtype == BF else 6
        u = torch.ones(B * N + 1, 2 * D, dtype=dtype, device="cuda")
        x = torch.ones(B * N + 1, D, dtype=dtype, device="cuda")
        out = torch.full((B * N + 1, 2 * D), 7.0, dtype=dtype, device="cuda")
        w, vec, ws = torch.ones(D, 15, device="cuda"), torch.ones(B * D, device="cuda"), torch.full((8192,), 7.0, device="cuda")
        st = stream()

        def taps(u_p, c_p, o_p, d_, k):         # the two launches that take the kernel size
            return (lib.htrvt_gnmixer_fwd(u_p, ptr(w), ptr(vec), o_p, ptr(ws), B, N, d_, k, dti, st),
                    lib.htrvt_gnmixer_bwd(u_p, c_p, c_p, ptr(w), ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(vec), o_p,
                                          ptr(ws), ptr(ws), B, N, d_, k, dti, st))

        def rest(c_p, o_p, d_):
            return (lib.htrvt_gnmixer_act(c_p, ptr(vec), ptr(vec), ptr(vec), ptr(vec), o_p, B, N, d_, dti, st),
                    lib.htrvt_gnmixer_bwd_reduce(c_p, c_p, ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(ws), ptr(ws), B, N, d_, dti, st))
        bad = {"even k": taps(ptr(u), ptr(x), ptr(out), D, 6), "k = 17": taps(ptr(u), ptr(x), ptr(out), D, 17),
               "k = 0": taps(ptr(u), ptr(x), ptr(out), D, 0),
               "C off the vector": taps(ptr(u), ptr(x), ptr(out), bad_d, 3) + rest(ptr(x), ptr(out), bad_d),
               "inputs unaligned": taps(ptr(u) + off, ptr(x) + off, ptr(out), D, 3) + rest(ptr(x) + off, ptr(out), D),
               "outputs unaligned": taps(ptr(u), ptr(x), ptr(out) + off, D, 3) + (
                   lib.htrvt_gnmixer_act(ptr(x), ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(out) + off, B, N, D, dti, st),),
               "dtype": (lib.htrvt_gnmixer_fwd(ptr(u), ptr(w), ptr(vec), ptr(out), ptr(ws), B, N, D, 3, 2, st),),
               "oversized grid": (lib.htrvt_gnmixer_fwd(ptr(u), ptr(w), ptr(vec), ptr(out), ptr(ws), 1 << 24, 4, 8 << 14, 3, dti, st),
                                  lib.htrvt_gnmixer_rows(1 << 24, 4, 8 << 14, dti)),
               "se D off the vector": (lib.htrvt_se_mean(ptr(x), ptr(ws), B, N, bad_d, dti, st),
                                       lib.htrvt_se_scale_fwd(ptr(x), ptr(vec), ptr(out), B, N, bad_d, dti, st),
                                       lib.htrvt_se_scale_bwd_reduce(ptr(x), ptr(x), ptr(ws), B, N, bad_d, dti, st),
                                       lib.htrvt_se_scale_bwd(ptr(x), ptr(vec), ptr(vec), ptr(out), B, N, bad_d, dti, st)),
               "se unaligned": (lib.htrvt_se_mean(ptr(x) + off, ptr(ws), B, N, D, dti, st),
                                lib.htrvt_se_scale_fwd(ptr(x), ptr(vec), ptr(out) + off, B, N, D, dti, st)),
               "resampling": (lib.htrvt_seq_down2_fwd(ptr(x), ptr(out), B, 1, D, dti, st),
                              lib.htrvt_seq_down2_fwd(ptr(x), ptr(out), B, N, bad_d, dti, st),
                              lib.htrvt_seq_down2_bwd(ptr(x), ptr(out) + off, B, N, D, dti, st),
                              lib.htrvt_seq_up_add_fwd(ptr(x), ptr(x), ptr(out), B, N + 1, N, D, dti, st),
                              lib.htrvt_seq_up_add_fwd(ptr(x), None, ptr(out), B, N // 2, N, D, dti, st),
                              lib.htrvt_seq_up_add_bwd(ptr(x), ptr(out), B, 0, N, D, dti, st)),
               "silu": (lib.htrvt_silu_fwd(ptr(x), ptr(out), 12 if dtype == BF else 6, dti, st),
                        lib.htrvt_silu_bwd(ptr(x), ptr(x) + off, ptr(out), 16, dti, st))}
        for what, rcs in bad.items():
            assert all(rc < 0 for rc in rcs), (what, rcs)
        assert lib.htrvt_last_error()
        torch.cuda.synchronize()
        assert (out == 7).all() and (ws == 7).all()


# ====================================================================== the autograd operators
def _leaf(t):
    return t.cuda().requires_grad_(True)


@pytest.mark.parametrize("B,N,Cc,k", [(2, 5, 8, 3), (3, 33, 24, 7), (5, 7, 40, 3)])
def test_glu_dwconv_gn_silu_against_float64_autograd(B, N, Cc, k):
    import htrvt_amd  # noqa: F401
    from htrvt_amd import variants
    u, ds, w, bias, gamma, beta = C.mixer_inputs(B, N, Cc, k, F32, seed=1)
    print(f"\nglu_dwconv_gn_silu B={B} N={N} C={Cc} k={k}")

    def ref(u_, w_, b_, ga_, be_, ds_):
        return (S.gn_mixer(u_, w_, b_, ga_, be_, B, N, EPS),) + tuple(S.grads_of(lambda *a: S.gn_mixer(*a, B, N, EPS), ds_, u_, w_, b_, ga_, be_))
    refs, errs = R.e32(ref, [u, w, bias, gamma, beta, ds])
    runs = []
    for _ in range(2):
        leaves = [_leaf(u), _leaf(w.view(Cc, 1, k)), _leaf(bias), _leaf(gamma), _leaf(beta)]
        s = variants.glu_dwconv_gn_silu(*leaves, B, N, EPS)
        s.backward(ds.cuda())
        runs.append([s.detach()] + [t.grad for t in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for n, g_, r_, e_ in zip(("s", "du", "dw", "dbias", "dgamma", "dbeta"), runs[0], refs, errs):
        _check(n, g_.reshape(r_.shape), r_, e_, False)


@pytest.mark.parametrize("B,N,D", [(1, 1, 8), (3, 33, 24)])
def test_squeeze_excite_against_float64_autograd(B, N, D):
    import htrvt_amd  # noqa: F401
    from htrvt_amd import variants
    x, dy, w1, b1, w2, b2 = C.se_inputs(B, N, D, F32, seed=1)
    print(f"\nsqueeze_excite B={B} N={N} D={D}")

    def ref(x_, w1_, b1_, w2_, b2_, dy_):
        return (S.se(x_, w1_, b1_, w2_, b2_, B, N),) + tuple(S.grads_of(lambda *a: S.se(*a, B, N), dy_, x_, w1_, b1_, w2_, b2_))
    refs, errs = R.e32(ref, [x, w1, b1, w2, b2, dy])
    runs = []
    for _ in range(2):
        leaves = [_leaf(t) for t in (x, w1, b1, w2, b2)]
        y = variants.squeeze_excite(*leaves, B, N)
        y.backward(dy.cuda())
        runs.append([y.detach()] + [t.grad for t in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for n, g_, r_, e_ in zip(("y", "dx", "dw1", "db1", "dw2", "db2"), runs[0], refs, errs):
        _check(n, g_, r_, e_, False)


@pytest.mark.parametrize("N0", [5, 33])
def test_resampling_operators_against_float64_autograd(N0):
    import htrvt_amd  # noqa: F401
    from htrvt_amd import variants
    B, D, n = 3, 24, N0 // 2
    g = torch.Generator().manual_seed(N0)
    x, skip, dout = [torch.randn(B * N0, D, generator=g) for _ in range(3)]
    print(f"\nresampling operators N0={N0}")
    xl, sl = _leaf(x), _leaf(skip)
    mid = variants.seq_downsample2(xl, B, N0)
    out = variants.seq_upsample_add(mid, sl, B, n, N0)
    (out * dout.cuda()).sum().backward()

    def ref(x_, s_, d_):
        return (S.up_add(S.down2(x_, B, N0), s_, B, n, N0),) + tuple(S.grads_of(lambda a, b: S.up_add(S.down2(a, B, N0), b, B, n, N0), d_, x_, s_))
    refs, errs = R.e32(ref, [x, skip, dout])
    for nme, g_, r_, e_ in zip(("out", "dx", "dskip"), (out, xl.grad, sl.grad), refs, errs):
        _check(nme, g_, r_, e_, False)
    one = x.cuda()[:B]
    assert variants.seq_downsample2(one, B, 1) is one           # N <= 1: the identity, no launch


# ====================================================================== the modules
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "squeezeformer.npz"))


_REFS = {}


def _reference(gold, case):
    """(x, dy, y, dx, grads) of a case in float64 over the fixture's state_dict, computed once"""
    if case not in _REFS:
        from htrvt_amd import conformer
        kind, args = C.CASES[case][:2]
        sd = C.case_module(conformer, case).state_dict()
        for (k, v), s in zip(sd.items(), gold[case + ".sdsum"]):
            assert abs(float(v.double().sum()) - float(s)) <= C.SUM_TOL * v.numel(), (case, k)
        x, dy = C.inputs(case)
        y, dx, grads = S.module_grads(kind, args, {k: v.double() for k, v in sd.items()}, x.double(), dy.double(), C.NORM_EPS,
                                      C.UP_TARGET.get(case))
        key = case + ".y" if case + ".y" in gold.files else None
        if key:                                             # small cases: the fork's own output, element by element
            assert float((y - torch.from_numpy(gold[key])).abs().max()) < 1e-10 * float(y.abs().max())
        _REFS[case] = (x, dy, y, dx, grads)
    return _REFS[case]


def _rel(name, got, ref, gate):
    ref = torch.as_tensor(ref, dtype=F64)
    err = float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max() / ref.abs().max())
    print(f"  {name}: {err:.2e} (gate {gate:.0e})")
    assert err < gate, (name, err)
    return err


@pytest.mark.parametrize("cdt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(C.CASES))
def test_module_reproduces_the_fork(gold, case, cdt):
    """outputs within 1e-3 of max |ref| and gradients within 2e-3 in float32; bfloat16 5e-2 / 1e-1.  One autograd node per
    forward; eval and train mode agree bit for bit (every rate is zero); two backward runs give the same bits."""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import conformer
    kind = C.CASES[case][0]
    go, gg = (1e-3, 2e-3) if cdt == F32 else (5e-2, 1e-1)
    x, dy, y_r, dx_r, g_r = _reference(gold, case)
    m = C.case_module(conformer, case, compute_dtype=cdt).cuda()
    extra = (C.UP_TARGET[case],) if kind == "up" else ()
    print(f"\n{case} {cdt}")
    with torch.no_grad():
        y_eval = m.eval()(x.cuda(), *extra)
    runs = []
    for _ in range(2):
        m.zero_grad()
        xr = x.cuda().requires_grad_(True)
        y = m.train()(xr, *extra)
        assert y.grad_fn is not None and y.grad_fn.name().startswith("_Function")
        assert y.dtype == F32 and xr.grad is None
        y.backward(dy.cuda())
        runs.append([y.detach(), xr.grad] + [p.grad.clone() for p in m.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(y_eval, runs[0][0])
    worst_g = _rel("dx", runs[0][1], dx_r, gg)
    _rel("y", runs[0][0], y_r, go)
    for (n, p), g_ in zip(m.named_parameters(), runs[0][2:]):
        assert g_.dtype == F32 and g_.shape == p.shape
        worst_g = max(worst_g, _rel("grad " + n, g_, g_r[n], gg))
    print(f"  worst gradient error {worst_g:.2e}")


def test_conv_module_dropout():
    """p = 0.1 on (3, 33, 64): the same seed gives the same output; every element of y_p - x is 0 or (y_0 - x) / (1 - p);
    the dropped share is within 5 sigma of p (sigma = sqrt(p (1 - p) / 6336) = 0.0038); the gradients are those of the
    float64 reference run with the recovered mask"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import conformer
    kind, args, kwargs, B, N = C.DROPOUT_CASE
    p, D = kwargs["dropout"], args[0]
    m = C.case_module(conformer, C.DROPOUT_CASE).cuda()
    sd64 = {k: v.double().cpu() for k, v in m.state_dict().items()}
    x, dy = [t.cuda() for t in C.inputs(None, C.DROPOUT_CASE)]
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
    with torch.no_grad():
        y0 = m.eval()(x)
    o_p, o_0 = (ys[0] - x).double().cpu().view(-1, D), (y0 - x).double().cpu().view(-1, D) / (1 - p)
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
    _, dx_r, g_r = S.module_grads(kind, args, sd64, x.double().cpu(), dy.double().cpu(), C.NORM_EPS, keep=keep, drop_p=p)
    _rel("dx", dx, dx_r, 2e-3)
    for n, g_ in grads.items():
        _rel("grad " + n, g_, g_r[n], 2e-3)
