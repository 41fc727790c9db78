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
  stem_stats sum / sum of squares 2.9e-8 .. 2.1e-5  5.4e-6 / 1.4e-7    0.38 / 0.33   (relative to the cancellation-free magnitude)
  stem_fwd y (float32 VALU)    6.6e-8 .. 2.1e-7   1.8e-7           0.17
  stem_fwd y (bfloat16 VALU)   1.1e-7 .. 1.8e-7   3.6e-3           0.99    (half a bfloat16 ulp just above a power of two)
  stem_fwd y (bfloat16 MFMA)   1.2e-7 .. 2.2e-7   2.9e-3           0.94    (gate: + the float16 operand bound, 4.9e-3 .. 5.1e-3 in all)

htrvt_stem_stats and htrvt_stem_fwd (the fused stem forward) follow at the end: the statistics against the float64 column
statistics relative to the cancellation-free magnitude, the three forward kernels (asserted by name) bit for bit on tied
grid data and on real-valued data with the arg-max bytes compared wherever the reference alone is certain (share left
out, largest case: float32 VALU 0.03 %, bfloat16 VALU 0.03 %, MFMA 0.62 %), and float32 against the unfused kernels.
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


# ====================================================================== the fused stem forward: batch statistics from the image
STATS_SHAPES = [(1, 2, 1),       # one conv row, one pixel
                (2, 4, 4),       # smallest regular case
                (3, 6, 37),      # a group of 3 rows, fewer than the 4 a block owns
                (2, 10, 4),      # two groups per image, the second holding one row
                (2, 64, 300),    # W above the 256 threads: the pixel loop runs twice
                (9, 64, 8)]      # 72 partial rows: the finishing kernel's unrolled-by-8 loop and its tail
STATS_C = [1, 24, 64, 520]       # 520: above the 512 threads of the finishing block


def _stem_stats_run(img, stats, w, u8):
    """htrvt_stem_stats -> colstats [2][C] on the host; the workspace has htrvt_stem_stats_rows rows of 64 floats, and the
    row behind it and the floats behind colstats keep their sentinel"""
    lib, check, ptr, stream, dt = _lib()
    B, H, W = img.shape
    C = w.shape[0]
    nrows = lib.htrvt_stem_stats_rows(B, H)
    assert nrows == B * ((H // 2 + 3) // 4)
    partial = torch.full((nrows + 1, 64), 99.0, device="cuda")
    col = torch.full((2 * C + 4,), 99.0, device="cuda")
    img_d, st_d, w_d = img.cuda(), stats.cuda(), w.cuda()
    check(lib.htrvt_stem_stats(ptr(img_d), ptr(st_d), ptr(w_d), ptr(partial), ptr(col), B, H, W, C, u8, stream()), "stem_stats")
    assert (partial[nrows] == 99).all() and (col[2 * C:] == 99).all()
    return col[:2 * C].view(2, C).cpu()


def _check_stem_stats(name, got, img, stats, w):
    """per channel, relative to the cancellation-free magnitude: |s1 - ref| <= 8 E32 sum_t |w_t| |X_t|,
    |s2 - ref| <= 8 E32 sum_tu |w_t| |w_u| |R_tu|; E32 = float32 error of the moments on these inputs, relative to max |R|"""
    (m64,), (e,) = R.e32(lambda i_, s_: torch.cat([t.flatten() for t in R.stem_moments(i_, s_)]), [img, stats])
    X, Rm = m64[:9], m64[9:].view(9, 9)
    e = e * float(m64.abs().max()) / float(Rm.abs().max())
    ref = R.stem_colstats(img.double() if img.is_floating_point() else img, stats.double(), w.double())
    aw = w.double().abs()
    mag = torch.stack([aw @ X.abs(), torch.einsum("ct,tu,cu->c", aw, Rm.abs(), aw)])
    obs = (got.double() - ref).abs() / mag
    print(f"  {name}: E32 {e:.2e}  gate {8 * e:.2e}  observed sum {float(obs[0].max()):.2e}  sum of squares {float(obs[1].max()):.2e}")
    return None if float(obs.max()) <= 8 * e else f"{name}: observed {float(obs.max()):.3e} of the cancellation-free magnitude is outside 8 * E32 = {8 * e:.3e}"


@pytest.mark.parametrize("u8", [0, 1])
@pytest.mark.parametrize("B,H,W", STATS_SHAPES)
def test_stem_stats(B, H, W, u8):
    """htrvt_stem_stats (stem_moments_kernel + stem_stats_kernel) against the float64 column statistics.  The gate of the
    channel sum is relative to |X_t|, itself a cancelling sum (at (2, 64, 300): |X_t| <= 11 against sum |x_t| = 13000, and
    float32 whitening alone moves X_t by 3e-4): the kernel meets it because it forms X in double from the pixels
    (float images 5.8e-8; uint8 images 5.4e-6, the float32 rounding of value / 255 that the kernels' contract fixes)"""
    g = _gen(B * 1000 + H * 10 + W + u8)
    img = _image(g, B, H, W, u8)
    stats = R.img_stats(img.reshape(B, -1), EPS, F64).float()
    print(f"\nstem_stats B={B} H={H} W={W} u8={u8}")
    bad = []
    for C in STATS_C:
        w = torch.randn(C, 9, generator=g) * 0.3
        bad.append(_check_stem_stats(f"stem colstats C={C}", _stem_stats_run(img, stats, w, u8), img, stats, w))
    assert not any(bad), [b for b in bad if b]


@pytest.mark.parametrize("u8", [0, 1])
def test_stem_stats_under_cancellation(u8):
    """smooth strokes beside ragged 1.0 padding and zero-sum (edge) filters: w.X and w^T R w are differences of large,
    nearly equal entries, and the gate stays relative to the entries"""
    import torch.nn.functional as F
    B, H, W, C = 3, 16, 64, 24
    g = _gen(12 + u8)
    x = torch.rand(B, 1, H, W, generator=g)
    for _ in range(3):
        x = F.avg_pool2d(F.pad(x, (4, 4, 4, 4), mode="replicate"), 9, stride=1)
    x = (x - x.amin()) / (x.amax() - x.amin())
    for b, cut in enumerate((25, 41, 64)):
        x[b, :, :, cut:] = 1.0
    img = (x[:, 0] * 255).round().to(torch.uint8) if u8 else x[:, 0].contiguous()
    stats = R.img_stats(img.reshape(B, -1), EPS, F64).float()
    w = torch.randn(C, 9, generator=g) * 0.3
    w[::2] -= w[::2].mean(dim=1, keepdim=True)
    print(f"\nstem_stats under cancellation u8={u8}")
    got = _stem_stats_run(img, stats, w, u8)
    ref = R.stem_colstats(img.double() if not u8 else img, stats.double(), w.double())
    X, Rm = R.stem_moments(img.double() if not u8 else img, stats.double())
    aw = w.double().abs()
    print(f"  result / cancellation-free magnitude, smallest: sum of squares {float((ref[1] / torch.einsum('ct,tu,cu->c', aw, Rm.abs(), aw)).min()):.1e}")
    bad = _check_stem_stats("stem colstats (cancelling)", got, img, stats, w)
    assert bad is None, bad


def test_stem_stats_refuses_bad_shapes_and_null_pointers_without_launching():
    lib, check, ptr, stream, dt = _lib()
    B, H, W, C = 2, 4, 4, 8
    img = torch.rand(B, 8, W, device="cuda")
    stats = torch.tensor([[0.5, 2.0]] * B, device="cuda")
    w = torch.ones(C, 9, device="cuda")
    partial = torch.full((8, 64), 7.0, device="cuda")
    col = torch.full((2, C), 7.0, device="cuda")
    args = [ptr(img), ptr(stats), ptr(w), ptr(partial), ptr(col)]
    for h, wd in ((5, W), (0, W), (H, 0)):
        assert lib.htrvt_stem_stats(*args, B, h, wd, C, 0, stream()) != 0, (h, wd)
    for k in range(5):
        a = list(args)
        a[k] = None
        assert lib.htrvt_stem_stats(*a, B, H, W, C, 0, stream()) != 0, k
    torch.cuda.synchronize()
    assert (partial == 7).all() and (col == 7).all()


# ====================================================================== the fused stem forward: all three kernels
MFMA, VALU_BF, VALU_F32 = "stem_mfma_fwd_kernel", "stem_fused_fwd_kernel<bf16_t>", "stem_fused_fwd_kernel<float>"


def _route(dtype, C):
    if dtype == F32:
        return VALU_F32
    return MFMA if C % 32 == 0 and C <= 512 else VALU_BF


def _stem_fwd_run(img, stats, w, scale, shift, dtype, u8, with_idx=True):
    """htrvt_stem_fwd -> y [B][Hp][W][C], idx (or None), on the device; asserts the kernel that served the launch and the
    sentinel rows behind both outputs"""
    lib, check, ptr, stream, dt = _lib()
    B, H, W = img.shape
    C = w.shape[0]
    Hp = R.pooled_rows(H // 2)
    y = torch.full((B * Hp * W + 1, C), 99.0, dtype=dtype, device="cuda")
    idx = torch.full((B * Hp * W + 1, C), 77, dtype=torch.uint8, device="cuda") if with_idx else None
    dev = [t.cuda() for t in (img, stats, w, scale, shift)]
    check(lib.htrvt_stem_fwd(*[ptr(t) for t in dev], ptr(y), ptr(idx), B, H, W, C, dt(dtype), u8, stream()), "stem_fwd")
    assert lib.htrvt_last_kernel().decode() == _route(dtype, C)
    assert (y[-1] == 99).all() and (idx is None or (idx[-1] == 77).all())
    return y[:-1].view(B, Hp, W, C), None if idx is None else idx[:-1].view(B, Hp, W, C)


W_VALU = [1, 2, 37, 300]                  # 1, 2: fewer pixels than threads per row (empty segments); 37, 300: uneven segments
W_MFMA = [1, 2, 30, 31, 37, 61, 121]      # blocks of 30 pixels: below one, exactly one, one + 1, three, five (wave 0 takes a second)
EXACT = ([(F32, C, W_VALU) for C in (4, 12, 64, 1024)] +          # 1024: 256 channel lanes, one thread walks the row; 12: 3 lanes
         [(BF, C, W_VALU) for C in (8, 24, 80, 544)] +            # 544: a multiple of 32 above 512, which the MFMA kernel declines
         [(BF, C, W_MFMA) for C in (32, 64, 96, 160, 512)])       # channel blocks 1, 3, 5: last single block; 2, 16: pair stores
POW2 = torch.tensor([0.25, 0.5, 1.0, 2.0])


def _signed_pow2(g, shape):
    return POW2[torch.randint(0, 4, shape, generator=g)] * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


@pytest.mark.parametrize("dtype,C,Ws", EXACT)
def test_stem_fwd_exact_on_tied_grid_data(dtype, C, Ws):
    """image on multiples of 0.25 in [-2, 2], statistics (0, 1), weights and scales signed powers of two, shifts on
    multiples of 0.5: every operand is exact in float16 and float32 and every accumulation exact, so values (rounded once to
    the output type) and arg-max bytes equal the float64 reference bit for bit -- first maximum in scan order among many
    ties, 15 exactly where the pooled value is not > 0 (exact zeros included).  H = 4: one pooled row, padding above;
    6: three conv rows, padding below the last pooled row; 10: five conv rows"""
    B = 2
    seen = torch.zeros(16, dtype=torch.long)
    zeros = 0
    for H in (4, 6, 10):
        for W in Ws:
            g = _gen(C * 10000 + H * 1000 + W)
            img = torch.randint(-8, 9, (B, H, W), generator=g).float() * 0.25
            stats = torch.tensor([[0.0, 1.0]] * B)
            w, scale = _signed_pow2(g, (C, 9)), _signed_pow2(g, (C,))
            shift = torch.randint(-6, 7, (C,), generator=g).float() * 0.5
            y_r, idx_r = R.stem_fwd(img.double(), stats.double(), w.double(), scale.double(), shift.double())
            y, idx = _stem_fwd_run(img, stats, w, scale, shift, dtype, 0)
            assert torch.equal(y.double().cpu(), y_r.to(dtype).double()), (H, W)
            assert torch.equal(idx.cpu(), idx_r), (H, W)
            y2, _ = _stem_fwd_run(img, stats, w, scale, shift, dtype, 0, with_idx=False)
            assert torch.equal(y2, y), (H, W)
            seen += torch.bincount(idx_r.flatten().long(), minlength=16)
            zeros += int((y_r == 0).sum())
    assert (seen[:9] > 0).all() and seen[15] > 0 and int(seen[9:15].sum()) == 0 and zeros > 0


REAL_SHAPES = [(2, 10, 37), (2, 8, 64), (3, 4, 31), (2, 64, 61)]
REAL_C = [(F32, 12), (F32, 1024), (BF, 24), (BF, 544), (BF, 32), (BF, 512)]


def _stem_real_inputs(g, B, H, W, C, u8):
    img = _image(g, B, H, W, u8)
    stats = R.img_stats(img.reshape(B, -1), EPS, F64).float()
    w = torch.randn(C, 9, generator=g) * 0.3
    gamma, beta = torch.randn(C, generator=g) + 1, torch.randn(C, generator=g) * 0.5
    out = R.conv1_fwd(img, stats.double(), w.double())[0]
    mean = out.mean((0, 1, 2))
    rstd = 1.0 / torch.sqrt(((out - mean) ** 2).mean((0, 1, 2)) + EPS)
    scale = (gamma.double() * rstd).float()
    shift = (beta.double() - mean * scale.double()).float()
    return img, stats, w, scale, shift


def _cells(t, fill):
    """[B][Hc][W][C] -> [B][Hp][W][C][9]: the nine cells of every pooling window, `fill` outside the tensor"""
    B, Hc, W, C = t.shape
    Hp = R.pooled_rows(Hc)
    pad = torch.full((B, Hc + 2, W + 2, C), fill, dtype=t.dtype)
    pad[:, 1:Hc + 1, 1:W + 1] = t
    return torch.stack([pad[:, r:r + 2 * Hp:2, c:c + W] for r in range(3) for c in range(3)], dim=-1)


def _real_cases():
    return [(d, C, B, H, W, (i + j) % 2) for j, (d, C) in enumerate(REAL_C) for i, (B, H, W) in enumerate(REAL_SHAPES)]


@pytest.mark.parametrize("dtype,C,B,H,W,u8", _real_cases())
def test_stem_fwd_on_real_valued_data(dtype, C, B, H, W, u8):
    """Values within the gate (for the MFMA kernel plus the window maximum of the float16 operand bound).  Bytes compared
    exactly where the float64 reference alone is certain: the window's largest BatchNorm output is positive by more than
    its gate and leads every other cell by more than the sum of their gates, or every cell is negative by more than its
    gate (byte 15).  Per-cell gate: 8 E32 max|ref| + 2^-19 |value| (the keyed bfloat16 rule treats values within 16
    float32 ulps as equal), plus the float16 bound for the MFMA kernel.  The share left out may be at most 1 % (VALU
    kernels) / 2 % (MFMA kernel)"""
    kern = _route(dtype, C)
    mfma = kern == MFMA
    g = _gen(C * 100 + H + W)
    img, stats, w, scale, shift = _stem_real_inputs(g, B, H, W, C, u8)
    print(f"\nstem_fwd {kern} C={C} B={B} H={H} W={W} u8={u8}")
    (y_r,), (ey,) = R.e32(lambda *a: R.stem_fwd(*a)[0], [img, stats, w, scale, shift])
    st64, w64, sc64, sh64 = stats.double(), w.double(), scale.double(), shift.double()
    out = R.conv1_fwd(img, st64, w64)[0]
    u = out * sc64 + sh64
    _, idx_r = R.bn_relu_maxpool(out, sc64, sh64)
    top = float(y_r.abs().max())
    gate = 8 * ey * top + 2.0 ** -19 * u.abs()
    tol = 8 * ey * top + (2.0 ** -8 * y_r.abs() if dtype == BF else 0.0)
    if mfma:
        fb = R.stem_f16_bound(img, st64, w64, sc64)
        gate = gate + fb
        tol = tol + _cells(fb, 0.0).amax(-1)
    cu, cg = _cells(u, float("-inf")), _cells(gate, 0.0)
    k = cu.argmax(-1, keepdim=True)
    ut, gt = cu.gather(-1, k), cg.gather(-1, k)
    lead = (ut - cu - gt - cg).scatter_(-1, k, float("inf"))
    sure_open = (ut > gt).squeeze(-1) & (lead.amin(-1) > 0)
    sure_closed = (cu < -cg).all(-1)
    sure = sure_open | sure_closed
    left_out = 1.0 - float(sure.double().mean())
    print(f"  bytes: left out {100 * left_out:.2f} %  closed windows {100 * float(sure_closed.double().mean()):.2f} %")
    assert left_out <= (0.02 if mfma else 0.01)
    assert sure_closed.any() and (idx_r[sure_closed] == 15).all()
    y, idx = _stem_fwd_run(img, stats, w, scale, shift, dtype, u8)
    d = (y.double().cpu() - y_r).abs()
    print(f"  stem y: E32 {ey:.2e}  gate {float(tol.max() if torch.is_tensor(tol) else tol) / top:.2e}  observed {float(d.max()) / top:.2e}"
          f"  observed / gate {float((d / tol).max()):.2f}")
    assert (d <= tol).all(), f"stem y: {float((d / tol).max()):.3f} of the gate"
    assert torch.equal(idx.cpu()[sure], idx_r[sure])
    y2, _ = _stem_fwd_run(img, stats, w, scale, shift, dtype, u8, with_idx=False)
    assert torch.equal(y2, y)


@pytest.mark.parametrize("B,H,W,C", [(2, 10, 37, 12), (2, 6, 300, 64)])
@pytest.mark.parametrize("u8", [0, 1])
def test_stem_fwd_float32_equals_the_unfused_kernels_bit_for_bit(B, H, W, C, u8):
    """the fused kernel keeps conv1_fwd_kernel's per-channel operation order: htrvt_stem_fwd == htrvt_conv1_fwd followed by
    htrvt_bn_relu_maxpool with the same scale and shift, values and bytes"""
    lib, check, ptr, stream, dt = _lib()
    g = _gen(C + W)
    img, stats, w, scale, shift = _stem_real_inputs(g, B, H, W, C, u8)
    y, idx = _stem_fwd_run(img, stats, w, scale, shift, F32, u8)
    Hc = H // 2
    Hp = R.pooled_rows(Hc)
    img_d, st_d, w_d, sc_d, sh_d = (t.cuda() for t in (img, stats, w, scale, shift))
    conv = torch.empty(B, Hc, W, C, device="cuda")
    col = torch.empty(B * Hc, 2, C, device="cuda")
    check(lib.htrvt_conv1_fwd(ptr(img_d), ptr(st_d), ptr(w_d), ptr(conv), ptr(col), B, H, W, C, dt(F32), u8, stream()), "conv1_fwd")
    y_u = torch.empty(B, Hp, W, C, device="cuda")
    idx_u = torch.empty(B, Hp, W, C, dtype=torch.uint8, device="cuda")
    check(lib.htrvt_bn_relu_maxpool(ptr(conv), ptr(sc_d), ptr(sh_d), ptr(y_u), ptr(idx_u), B, Hc, W, C, dt(F32), stream()), "bn_relu_maxpool")
    assert torch.equal(y, y_u) and torch.equal(idx, idx_u)
    assert (idx_u == 15).any() and (idx_u < 9).any()


def test_stem_fwd_refuses_unsupported_shapes_and_null_pointers_without_launching():
    """a channel count that is not whole 16-byte vectors, odd H, H = 2 (no pooled row of two conv rows), a null pointer:
    non-zero, outputs untouched, htrvt_last_kernel() unchanged"""
    lib, check, ptr, stream, dt = _lib()
    B, W = 2, 4
    img = torch.rand(B, 8, W, device="cuda")
    stats = torch.tensor([[0.5, 2.0]] * B, device="cuda")
    vec = torch.ones(64 * 9, device="cuda")
    before = lib.htrvt_last_kernel()
    for dtype, C, H, null in ((BF, 12, 4, None), (F32, 6, 4, None), (BF, 32, 5, None), (F32, 8, 5, None), (BF, 32, 2, None), (BF, 8, 2, None),
                              (F32, 8, 2, None)) + tuple((d, C, 4, k) for d, C in ((BF, 32), (BF, 8), (F32, 8)) for k in range(6)):
        y = torch.full((B * 2 * W, 64), 7.0, dtype=dtype, device="cuda")
        idx = torch.full((B * 2 * W, 64), 7, dtype=torch.uint8, device="cuda")
        a = [ptr(img), ptr(stats), ptr(vec), ptr(vec), ptr(vec), ptr(y)]
        if null is not None:
            a[null] = None
        assert lib.htrvt_stem_fwd(*a, ptr(idx), B, H, W, C, dt(dtype), 0, stream()) != 0, (dtype, C, H, null)
        torch.cuda.synchronize()
        assert (y == 7).all() and (idx == 7).all(), (dtype, C, H, null)
    assert lib.htrvt_last_kernel() == before
