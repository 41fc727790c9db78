"""The stem's HBM-bound kernels through the C ABI against tests/kernel_refs.py: BatchNorm + ReLU + max-pool and its
backward (exact, on tied integer data: the arg-max byte must be ATen's first maximum in scan order, 15 where the ReLU
is closed), the image statistics, conv1 forward with its column statistics, the conv1 weight gradient, and the fused
conv1 -> BatchNorm -> ReLU -> max-pool backward against the unfused chain's reference AND float64 autograd.

Non-exact comparisons: per element against the float64 reference over the same (already rounded) inputs, relative to the
reference's largest magnitude, gate = 8 * E32 (+ 2^-8 |ref| for a bfloat16 output), E32 = the float32 evaluation error of
the reference itself on these inputs (kernel_refs.e32).

Every non-exact comparison prints its E32, gate and observed error (`pytest -s`).  Measured on an MI355X, over all
parametrised cases of an output (errors relative to max |ref|; a bfloat16 gate is 2^-8 = 3.9e-3 plus 8 * E32):

  output                       E32 (range)        worst observed   worst observed / gate
  pooled (real-valued) bf16/f32 4.5e-8 .. 5.6e-8  2.0e-3 / 2.4e-8  0.51 / 0.07
  img_stats                    2.5e-8 .. 1.1e-7   8.3e-8           0.21
  conv1 out           bf16     8.1e-8 .. 2.2e-7   3.6e-3           0.93
  conv1 out           f32      6.8e-8 .. 2.0e-7   2.0e-7           0.13
  conv1 colstats               7.2e-8 .. 2.8e-7   5.6e-7           0.42
  conv1_wgrad dw               8.2e-8 .. 3.9e-6   5.6e-7           0.18
  conv1_bwd vs chain: dw       6.8e-8 .. 3.3e-6   3.0e-7           0.17
  conv1_bwd vs chain: dgamma / dbeta 1.0e-8 .. 4.1e-7  2.5e-7 / 2.0e-7  0.26 / 0.56
  conv1_bwd vs autograd: dw    7.3e-8 .. 1.0e-2   2.7e-7           0.22    (the float32 autograd run flips arg-maxes)
  conv1_bwd vs autograd: dgamma / dbeta 1.0e-8 .. 3.3e-7  2.6e-7 / 2.0e-7  0.22 / 0.62
"""
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
EPS = float(torch.tensor(1e-5, dtype=F32))           # the value the float argument of the entry points carries
SET = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import dt, ptr, stream
    return lib, check, ptr, stream, dt


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, got, ref, err, bf16_out):
    ok, obs = R.gate_check(name, got.detach().cpu(), ref, err, bf16_out)
    assert ok, f"{name}: observed {obs:.3e} of max|ref| is outside 8 * E32 = {8 * err:.3e}" + (" + one bf16 ulp" if bf16_out else "")


# ====================================================================== BatchNorm + ReLU + max-pool and its backward (exact)
@pytest.mark.parametrize("W", [1, 2, 37])
@pytest.mark.parametrize("H", [1, 2, 5, 32])
@pytest.mark.parametrize("dtype,C", [(BF, 8), (BF, 24), (BF, 64), (F32, 4), (F32, 12)])
def test_maxpool_pair_on_tied_data(dtype, C, H, W):
    """data on the grid -2 .. 2: nearly every window holds its maximum several times.  Pooled values, arg-max bytes (first
    maximum in (row, column) scan order; 15 exactly where a scale is given and the pooled value is not > 0) and the
    backward fed with the forward's own bytes, all bit for bit; scale NULL = plain max-pool; idx NULL"""
    lib, check, ptr, stream, dt = _lib()
    B = 3
    g = _gen(H * 1000 + W * 10 + C)
    Ho = R.pooled_rows(H)
    x = torch.randint(-2, 3, (B, H, W, C), generator=g).float()
    scale = torch.tensor(SET)[torch.randint(0, 6, (C,), generator=g)]
    shift = torch.randint(-3, 4, (C,), generator=g).float() * 0.5
    dpool = torch.randint(-8, 9, (B, Ho, W, C), generator=g).float()
    x_d, sc_d, sh_d, dp_d = x.to(dtype).cuda(), scale.cuda(), shift.cuda(), dpool.to(dtype).cuda()
    seen = torch.zeros(16, dtype=torch.long)
    for with_bn in (False, True):
        sc, sh = (scale.double(), shift.double()) if with_bn else (None, None)
        y_r, idx_r = R.bn_relu_maxpool(x.double(), sc, sh)
        y = torch.full((B * Ho * W + 1, C), 99.0, dtype=dtype, device="cuda")
        idx = torch.full((B * Ho * W + 1, C), 77, dtype=torch.uint8, device="cuda")
        check(lib.htrvt_bn_relu_maxpool(ptr(x_d), ptr(sc_d) if with_bn else None, ptr(sh_d) if with_bn else None, ptr(y), ptr(idx),
                                        B, H, W, C, dt(dtype), stream()), "bn_relu_maxpool")
        assert torch.equal(y[:-1].double().cpu().view(B, Ho, W, C), y_r)
        assert torch.equal(idx[:-1].cpu().view(B, Ho, W, C), idx_r)
        assert (y[-1] == 99).all() and (idx[-1] == 77).all()
        assert (idx_r == 15).any() == (with_bn and bool((y_r <= 0).any()))
        seen += torch.bincount(idx_r.flatten().long(), minlength=16)
        y2 = torch.empty(B * Ho * W, C, dtype=dtype, device="cuda")
        check(lib.htrvt_bn_relu_maxpool(ptr(x_d), ptr(sc_d) if with_bn else None, ptr(sh_d) if with_bn else None, ptr(y2), None,
                                        B, H, W, C, dt(dtype), stream()), "bn_relu_maxpool without idx")
        assert torch.equal(y2, y[:-1])
        # backward through the forward's own bytes
        gin = torch.full((B * H * W + 1, C), 99.0, dtype=dtype, device="cuda")
        check(lib.htrvt_maxpool_bwd(ptr(dp_d), ptr(idx), ptr(x_d), ptr(sc_d) if with_bn else None, ptr(sh_d) if with_bn else None,
                                    ptr(gin), B, H, W, C, dt(dtype), stream()), "maxpool_bwd")
        g_r = R.maxpool_bwd(dpool.double(), idx_r, x.double(), sc, sh)
        assert torch.equal(gin[:-1].double().cpu().view(B, H, W, C), g_r)
        assert (gin[-1] == 99).all()
    if H >= 5 and W == 37:
        assert (seen[:9] > 0).all(), "every window position should win somewhere"


def test_maxpool_pair_refuses_unsupported_widths_without_launching():
    lib, check, ptr, stream, dt = _lib()
    B, H, W = 1, 2, 2
    for dtype, C in ((BF, 12), (F32, 6)):
        x = torch.ones(B, H, W, C, dtype=dtype, device="cuda")
        out = torch.full((B, H, W, C), 7.0, dtype=dtype, device="cuda")
        idx = torch.full((B, H, W, C), 7, dtype=torch.uint8, device="cuda")
        assert lib.htrvt_bn_relu_maxpool(ptr(x), None, None, ptr(out), ptr(idx), B, H, W, C, dt(dtype), stream()) != 0
        assert lib.htrvt_maxpool_bwd(ptr(x), ptr(idx), ptr(x), None, None, ptr(out), B, H, W, C, dt(dtype), stream()) != 0
        torch.cuda.synchronize()
        assert (out == 7).all() and (idx == 7).all()


@pytest.mark.parametrize("dtype,C", [(BF, 24), (F32, 12)])
def test_maxpool_on_real_valued_data(dtype, C):
    """pooled values within the gate; bytes compared where the float64 window maximum leads the runner-up by more than the
    gate (the one stated exception: at most 1 % of the elements may be left out)"""
    lib, check, ptr, stream, dt = _lib()
    B, H, W = 2, 32, 37
    g = _gen(C)
    x = torch.randn(B, H, W, C, generator=g).to(dtype)
    scale, shift = torch.randn(C, generator=g) + 1.5, torch.randn(C, generator=g) * 0.3
    print(f"\nmaxpool real-valued {dtype} C={C}")
    (y_r,), (ey,) = R.e32(lambda a, b, c: R.bn_relu_maxpool(a, b, c)[0], [x.float(), scale, shift])
    _, idx_r = R.bn_relu_maxpool(x.double(), scale.double(), shift.double())
    # from the reference alone: a byte is certain where the window's largest BatchNorm output is positive and leads the
    # runner-up by more than the gate (an open ReLU, a clear winner) or where it is negative by more than the gate (15)
    u = x.double() * scale.double() + shift.double()
    Ho = R.pooled_rows(H)
    pad = torch.full((B, H + 2, W + 2, C), float("-inf"), dtype=F64)
    pad[:, 1:H + 1, 1:W + 1] = u
    cells = torch.stack([pad[:, r:r + 2 * Ho:2, c:c + W] for r in range(3) for c in range(3)], dim=-1)
    top2 = cells.topk(2, dim=-1).values
    tol = 8 * ey * float(y_r.abs().max())
    sure = ((top2[..., 0] > tol) & (top2[..., 0] - top2[..., 1] > tol)) | (top2[..., 0] < -tol)
    assert float((~sure).float().mean()) <= 0.01
    assert (idx_r[top2[..., 0] < -tol] == 15).all() and (idx_r == 15).any()
    x_d, sc_d, sh_d = x.cuda(), scale.cuda(), shift.cuda()
    y = torch.empty(B, Ho, W, C, dtype=dtype, device="cuda")
    idx = torch.empty(B, Ho, W, C, dtype=torch.uint8, device="cuda")
    check(lib.htrvt_bn_relu_maxpool(ptr(x_d), ptr(sc_d), ptr(sh_d), ptr(y), ptr(idx), B, H, W, C, dt(dtype), stream()), "bn_relu_maxpool")
    _check("pooled", y.float(), y_r, ey, dtype == BF)
    assert torch.equal(idx.cpu()[sure], idx_r[sure])


# ====================================================================== image statistics
@pytest.mark.parametrize("u8", [0, 1])
@pytest.mark.parametrize("H,W", [(4, 4), (4, 37), (6, 4), (10, 512), (64, 512), (64, 37)])
def test_img_stats(H, W, u8):
    lib, check, ptr, stream, dt = _lib()
    B = 3
    g = _gen(H * W + u8)
    img = torch.randint(0, 256, (B, H * W), generator=g).to(torch.uint8) if u8 else torch.rand(B, H * W, generator=g) * 0.2 + 0.7
    print(f"\nimg_stats H={H} W={W} u8={u8}")
    st_r = R.img_stats(img, EPS, F64)
    es = float((R.img_stats(img, EPS, F32).double() - st_r).abs().max() / st_r.abs().max())
    img_d = img.cuda()
    stats = torch.full((B + 1, 2), 7.0, device="cuda")
    check(lib.htrvt_img_stats(ptr(img_d), ptr(stats), B, H * W, EPS, u8, stream()), "img_stats")
    _check("img_stats", stats[:B], st_r, es, False)
    assert (stats[B] == 7).all()


def test_img_stats_refuses_a_pixel_count_that_is_not_a_multiple_of_4():
    lib, check, ptr, stream, dt = _lib()
    img = torch.ones(2, 222, device="cuda")
    stats = torch.full((2, 2), 7.0, device="cuda")
    assert lib.htrvt_img_stats(ptr(img), ptr(stats), 2, 222, EPS, 0, stream()) != 0
    torch.cuda.synchronize()
    assert (stats == 7).all()


# ====================================================================== conv1
def _image(g, B, H, W, u8):
    """a line image: bright paper, dark strokes -- uint8, or float32 in [0, 1]"""
    img = torch.rand(B, H, W, generator=g) * 0.3 + 0.7
    img[torch.rand(B, H, W, generator=g) < 0.15] = 0.1
    if u8:
        return (img * 255).round().to(torch.uint8)
    return img


# channel vectors per pixel 1, 2, 3, 6, 12, 24, 64: conv1_bwd's channel lanes per wave 1, 2, 1, 2, 4, 8, 8; 256 % {3, 6, 12, 24} != 0
CONV_C = {BF: [8, 16, 24, 48, 96, 192, 512], F32: [4, 8, 12, 24, 48, 96, 256]}
CONV_HW = [(4, 4), (6, 37), (10, 4), (64, 37), (10, 512)]


def _conv_cases():
    out = []
    for d in (BF, F32):
        for i, C in enumerate(CONV_C[d]):
            for j, (H, W) in enumerate(CONV_HW):
                out.append((d, C, H, W, (i + j) % 2))
    return out


@pytest.mark.parametrize("dtype,C,H,W,u8", _conv_cases())
def test_conv1_forward_and_weight_gradient(dtype, C, H, W, u8):
    lib, check, ptr, stream, dt = _lib()
    B = 2
    g = _gen(C * 100 + H + W)
    bf = dtype == BF
    img = _image(g, B, H, W, u8)
    stats = R.img_stats(img.reshape(B, -1), EPS, F64).float()             # an input of the conv kernels
    w = torch.randn(C, 9, generator=g) * 0.3
    Hc = H // 2
    print(f"\nconv1 {dtype} C={C} H={H} W={W} u8={u8}")
    (out_r, col_r), (eo, ec) = R.e32(R.conv1_fwd, [img, stats, w])
    img_d, st_d, w_d = img.cuda(), stats.cuda(), w.cuda()
    out = torch.full((B * Hc * W + 1, C), 99.0, dtype=dtype, device="cuda")
    col = torch.full((B * Hc + 1, 2, C), 99.0, device="cuda")
    check(lib.htrvt_conv1_fwd(ptr(img_d), ptr(st_d), ptr(w_d), ptr(out), ptr(col), B, H, W, C, dt(dtype), u8, stream()), "conv1_fwd")
    _check("conv1 out", out[:-1].float().view(B, Hc, W, C), out_r, eo, bf)
    _check("conv1 colstats", col[:-1], col_r, ec, False)
    assert (out[-1] == 99).all() and (col[-1] == 99).all()

    dy = torch.randn(B, Hc, W, C, generator=g).to(dtype)
    dw0 = torch.randn(C, 9, generator=g)
    (dw_r,), (edw,) = R.e32(lambda a, b, c, d: R.conv1_wgrad(a, b, c) + d, [img, stats, dy.float(), dw0])
    nblk = lib.htrvt_conv1_wgrad_blocks(B, H)
    assert nblk == min(B * Hc, 512)
    dy_d = dy.cuda()
    dw = torch.cat([dw0.flatten(), torch.full((9,), 99.0)]).cuda()
    partial = torch.full((nblk + 1, C * 9), 99.0, device="cuda")
    check(lib.htrvt_conv1_wgrad(ptr(img_d), ptr(st_d), ptr(dy_d), ptr(dw), ptr(partial), B, H, W, C, dt(dtype), u8, stream()), "conv1_wgrad")
    _check("conv1 dw", dw[:C * 9].view(C, 9), dw_r, edw, False)
    assert (dw[C * 9:] == 99).all() and (partial[nblk] == 99).all()


def test_conv1_weight_gradient_above_its_block_cap():
    """B * H/2 = 640 output rows over 512 blocks: blocks loop over rows"""
    lib, check, ptr, stream, dt = _lib()
    B, H, W, C = 20, 64, 8, 24
    g = _gen(1)
    img = _image(g, B, H, W, 1)
    stats = R.img_stats(img.reshape(B, -1), EPS, F64).float()
    dy = torch.randn(B, H // 2, W, C, generator=g).to(BF)
    print("\nconv1_wgrad 640 rows")
    (dw_r,), (edw,) = R.e32(R.conv1_wgrad, [img, stats, dy.float()])
    nblk = lib.htrvt_conv1_wgrad_blocks(B, H)
    assert nblk == 512
    img_d, st_d, dy_d = img.cuda(), stats.cuda(), dy.cuda()
    dw = torch.zeros(C, 9, device="cuda")
    partial = torch.empty(nblk, C * 9, device="cuda")
    check(lib.htrvt_conv1_wgrad(ptr(img_d), ptr(st_d), ptr(dy_d), ptr(dw), ptr(partial), B, H, W, C, 1, 1, stream()), "conv1_wgrad")
    _check("conv1 dw", dw, dw_r, edw, False)


@pytest.mark.parametrize("dtype,C,H,W,u8", _conv_cases())
def test_conv1_fused_backward(dtype, C, H, W, u8):
    """htrvt_conv1_bwd over the reference's arg-max bytes (an INPUT of the kernel): dw, dgamma, dbeta accumulated into
    non-zero buffers, against the unfused chain (max-pool backward through the bytes, BatchNorm backward, conv1 weight
    gradient) in float64 over the same inputs, and against float64 autograd of conv -> BN(train) -> ReLU -> max_pool2d"""
    lib, check, ptr, stream, dt = _lib()
    B = 2
    g = _gen(C * 100 + H + W + 7)
    img = _image(g, B, H, W, u8)
    stats = R.img_stats(img.reshape(B, -1), EPS, F64).float()
    w = torch.randn(C, 9, generator=g) * 0.3
    gamma, beta = torch.randn(C, generator=g) + 1, torch.randn(C, generator=g) * 0.5
    Hc = H // 2
    Hp = R.pooled_rows(Hc)
    dpool = torch.randn(B, Hp, W, C, generator=g).to(dtype)
    acc0 = [torch.randn(C, 9, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)]
    print(f"\nconv1_bwd {dtype} C={C} H={H} W={W} u8={u8}")

    def auto(st_, w_, ga_, be_, dp_, a0, a1, a2):
        dw_, dg_, db_, y_, m_, r_ = R.conv1_chain_autograd(img, st_, w_, ga_, be_, dp_, EPS)
        return dw_ + a0, dg_ + a1, db_ + a2, y_, m_, r_
    (dw_a, dg_a, db_a, y64, mean64, rstd64), ea = R.e32(auto, [stats, w, gamma, beta, dpool.float()] + acc0)
    mean, rstd = mean64.float(), rstd64.float()                           # inputs of the kernel: the saved batch statistics
    sc64 = gamma.double() * rstd64
    _, idx = R.bn_relu_maxpool(y64, sc64, beta.double() - mean64 * sc64)  # the bytes the forward would have written

    def chain(st_, w_, ga_, m_, r_, dp_, a0, a1, a2):
        dw_, dg_, db_ = R.conv1_chain_unfused(img, st_, w_, ga_, m_, r_, dp_, idx)
        return dw_ + a0, dg_ + a1, db_ + a2
    (dw_c, dg_c, db_c), ec = R.e32(chain, [stats, w, gamma, mean, rstd, dpool.float()] + acc0)

    nrows, ld = lib.htrvt_conv1_bwd_rows(B, H), lib.htrvt_conv1_bwd_row_floats(C)
    img_d, st_d, w_d, ga_d, m_d, r_d, dp_d, idx_d = (t.cuda() for t in (img, stats, w, gamma, mean, rstd, dpool, idx))
    partial = torch.full((nrows + 1, ld), 99.0, device="cuda")
    dw, dg, db = (torch.cat([a.flatten(), torch.full((4,), 99.0)]).cuda() for a in acc0)
    check(lib.htrvt_conv1_bwd(ptr(img_d), ptr(st_d), ptr(dp_d), ptr(idx_d), ptr(w_d), ptr(ga_d), ptr(m_d), ptr(r_d), ptr(partial),
                              ptr(dw), ptr(dg), ptr(db), B, H, W, C, dt(dtype), u8, stream()), "conv1_bwd")
    assert (partial[nrows] == 99).all() and (dw[-4:] == 99).all() and (dg[-4:] == 99).all() and (db[-4:] == 99).all()
    _check("chain dw", dw[:-4].view(C, 9), dw_c, ec[0], False)
    _check("chain dgamma", dg[:-4], dg_c, ec[1], False)
    _check("chain dbeta", db[:-4], db_c, ec[2], False)
    _check("autograd dw", dw[:-4].view(C, 9), dw_a, ea[0], False)
    _check("autograd dgamma", dg[:-4], dg_a, ea[1], False)
    _check("autograd dbeta", db[:-4], db_a, ea[2], False)


def test_conv1_entry_points_refuse_unsupported_shapes_without_launching():
    """conv1_bwd: more than 8 waves per block or a channel count that is not whole 16-byte vectors -- refused before the
    first of its three launches (as the finalize kernel's LDS limit is, which only channel counts above the wave limit
    could reach), so the scratch stays untouched"""
    lib, check, ptr, stream, dt = _lib()
    B, H, W = 1, 4, 4
    img = torch.rand(B, H, W, device="cuda")
    stats = torch.tensor([[0.5, 2.0]], device="cuda")
    for dtype, C in ((BF, 1024), (F32, 512), (F32, 6), (BF, 12)):       # 128 vectors of 16 bytes / 8 channel lanes = 16 waves
        vec = torch.ones(C * 9, device="cuda")
        dpool = torch.ones(B, 1, W, C, dtype=dtype, device="cuda")
        idx = torch.zeros(B, 1, W, C, dtype=torch.uint8, device="cuda")
        nrows, ld = lib.htrvt_conv1_bwd_rows(B, H), lib.htrvt_conv1_bwd_row_floats(C)
        partial = torch.full((nrows, ld), 7.0, device="cuda")
        outs = torch.full((3, C * 9), 7.0, device="cuda")
        rc = lib.htrvt_conv1_bwd(ptr(img), ptr(stats), ptr(dpool), ptr(idx), ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(partial),
                                 ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), B, H, W, C, dt(dtype), 0, stream())
        torch.cuda.synchronize()
        assert rc != 0 and (partial == 7).all() and (outs == 7).all(), (dtype, C)
        if C % (8 if dtype == BF else 4):
            out = torch.full((B, H // 2, W, C), 7.0, dtype=dtype, device="cuda")
            col = torch.full((B * H // 2, 2, C), 7.0, device="cuda")
            assert lib.htrvt_conv1_fwd(ptr(img), ptr(stats), ptr(vec), ptr(out), ptr(col), B, H, W, C, dt(dtype), 0, stream()) != 0
            assert lib.htrvt_conv1_wgrad(ptr(img), ptr(stats), ptr(out), ptr(outs[0]), ptr(partial), B, H, W, C, dt(dtype), 0, stream()) != 0
            torch.cuda.synchronize()
            assert (out == 7).all() and (col == 7).all() and (outs == 7).all()
