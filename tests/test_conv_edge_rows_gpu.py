"""3x3 / pad-1 convolutions at the image heights where kernel rows fall into the zero padding.

The halo forward / dgrad kernels (csrc/gemm_halo_impl.h) walk only the kernel rows that read the image, and the
halo-staged weight-gradient kernels (csrc/gemm_hwgrad_impl.h) skip the k-tiles of output rows whose x row is padding.
The skipped terms are exact zeros, so everything here is an exact comparison on integer-valued data against
F.conv2d autograd (the style of tests/test_gemm_gpu.py), at heights 1, 2, 3, 4 and 8 -- one, two or no kernel rows in
the padding per tile -- and with split-K ranges that start mid-row or hold no live k-tile at all.  Every case asserts
through htrvt_last_kernel() that the intended kernel served it."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _ops():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import ops
    return ops


def _last_kernel():
    from htrvt_amd._lib import lib
    return lib.htrvt_last_kernel().decode()


def _ints(shape, lo=-2, hi=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).double()


def _pack_fwd(w, cp):      # [Co,Ci,kh,kw] -> [Co][taps][Cpad]
    Co, Ci, kh, kw = w.shape
    out = torch.zeros(Co, kh * kw, cp, dtype=w.dtype)
    out[:, :, :Ci] = w.permute(0, 2, 3, 1).reshape(Co, kh * kw, Ci)
    return out


def _pack_dgrad(w, cp):    # [Co,Ci,kh,kw] -> [Ci][taps][Cpad(Co)]
    Co, Ci, kh, kw = w.shape
    out = torch.zeros(Ci, kh * kw, cp, dtype=w.dtype)
    out[:, :, :Co] = w.permute(1, 2, 3, 0).reshape(Ci, kh * kw, Co)
    return out


@functools.lru_cache(maxsize=4)
def _reference(Bn, Hi, Wi, C, stride):
    """x, w, y, dy (NCHW, float64, integer-valued) and the autograd gradients of F.conv2d"""
    x = _ints((Bn, C, Hi, Wi), seed=10 + Hi).requires_grad_(True)
    w = _ints((C, C, 3, 3), seed=11).requires_grad_(True)
    y = F.conv2d(x, w, None, stride=stride, padding=1)
    dy = _ints(tuple(y.shape), seed=12 + Hi)
    y.backward(dy)
    return x.detach(), w.detach(), y.detach(), dy, x.grad, w.grad


HEIGHTS = [1, 2, 3, 4, 8]


# --------------------------------------------------------------------------------------------------------------------
# forward and plain dgrad, bf16 and float32 results
# --------------------------------------------------------------------------------------------------------------------
# tile 12 asks for the halo kernel with the 192-column tile the training shapes take; on its own the library gives these
# few-pixel problems 128-column tiles at 384 channels (pick_bn, csrc/gemm_dma.hip)
@pytest.mark.parametrize("tile", [0, 12])
@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("Wi", [256, 512])
@pytest.mark.parametrize("Hi", HEIGHTS)
def test_halo_fwd_dgrad_edge_rows_exact(Hi, Wi, C, tile):
    ops = _ops()
    Bn = 2
    bn = 192 if (C == 192 or tile == 12) else 128
    x, w, y, dy, gx, _ = _reference(Bn, Hi, Wi, C, (1, 1))
    geom = ops.ConvGeom(Bn, Hi, Wi, C, C, 3, (1, 1), 1)
    M, cp = Bn * Hi * Wi, ops.cpad(C, BF)
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    wf, wd = _pack_fwd(w, cp).to(BF).cuda(), _pack_dgrad(w, cp).to(BF).cuda()
    y_nhwc, gx_nhwc = y.permute(0, 2, 3, 1), gx.permute(0, 2, 3, 1)
    nmt = ops.gemm_num_mtiles(M, C, BF, gather=ops.GATHER_CONV_FWD)
    for f32 in (False, True):
        odt = torch.float32 if f32 else BF
        tag = ", f32>" if f32 else ">"
        cs = torch.zeros(nmt, 2, C, dtype=torch.float32, device="cuda")
        yd = torch.full((Bn, Hi, Wi, C), 7.0, dtype=odt, device="cuda")
        ops.gemm(xd, wf, yd, dtype=BF, M=M, N=C, K=9 * cp, lda=C, ldb=9 * cp, ldc=C, gather=ops.GATHER_CONV_FWD, geom=geom,
                 Cpad=cp, colstats=cs, c_f32=f32, tile=tile)
        assert _last_kernel() == f"gemm_halo_kernel<{bn}, false" + tag, _last_kernel()
        assert torch.equal(yd.double().cpu(), y_nhwc.to(odt).double())
        assert torch.equal(cs[:, 0].double().sum(0).cpu(), y_nhwc.reshape(-1, C).sum(0))
        assert torch.allclose(cs[:, 1].double().sum(0).cpu(), (y_nhwc.reshape(-1, C) ** 2).sum(0), rtol=1e-6, atol=1e-3)
        dxd = torch.full((Bn, Hi, Wi, C), 7.0, dtype=odt, device="cuda")
        ops.gemm(dyd, wd, dxd, dtype=BF, M=M, N=C, K=9 * cp, lda=C, ldb=9 * cp, ldc=C, gather=ops.GATHER_CONV_DGRAD, geom=geom,
                 Cpad=cp, c_f32=f32, tile=tile)
        assert _last_kernel() == f"gemm_halo_kernel<{bn}, true" + tag, _last_kernel()
        assert torch.equal(dxd.double().cpu(), gx_nhwc.to(odt).double())


# forward with a row stride of 2 (layer1.0.conv1): one output row (Hi = 2), an odd height whose bottom output row reads the
# padding (Hi = 3), and the training shape (Hi = 16), where only the top output row has a kernel row in the padding
@pytest.mark.parametrize("Hi", [2, 3, 16])
def test_halo_fwd_row_stride2_edge_rows_exact(Hi):
    ops = _ops()
    Bn, Wi, C = 2, 256, 192
    x, w, y, _, _, _ = _reference(Bn, Hi, Wi, C, (2, 1))
    geom = ops.ConvGeom(Bn, Hi, Wi, C, C, 3, (2, 1), 1)
    M, cp = Bn * geom.Ho * geom.Wo, ops.cpad(C, BF)
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    wf = _pack_fwd(w, cp).to(BF).cuda()
    yd = torch.full((Bn, geom.Ho, geom.Wo, C), 7.0, dtype=BF, device="cuda")
    cs = torch.zeros(ops.gemm_num_mtiles(M, C, BF, gather=ops.GATHER_CONV_FWD), 2, C, dtype=torch.float32, device="cuda")
    ops.gemm(xd, wf, yd, dtype=BF, M=M, N=C, K=9 * cp, lda=C, ldb=9 * cp, ldc=C, gather=ops.GATHER_CONV_FWD, geom=geom,
             Cpad=cp, colstats=cs)
    assert _last_kernel() == "gemm_halo_kernel<192, false>", _last_kernel()
    y_nhwc = y.permute(0, 2, 3, 1)
    assert torch.equal(yd.double().cpu(), y_nhwc.to(BF).double())
    assert torch.equal(cs[:, 0].double().sum(0).cpu(), y_nhwc.reshape(-1, C).sum(0))


# forward with stride (2,2) (conv1 of layer2.0 / layer3.0, gemm_halo_fs2_kernel): the same skip over its (kernel row, chunk)
# units -- one output row (Hi = 2), an odd height (both ends in the padding), the training height of layer 3.0 (Hi = 4)
@pytest.mark.parametrize("Hi", [2, 3, 4])
def test_halo_fwd_stride22_edge_rows_exact(Hi):
    ops = _ops()
    Bn, Wi, C = 2, 512, 192
    x, w, y, _, _, _ = _reference(Bn, Hi, Wi, C, (2, 2))
    geom = ops.ConvGeom(Bn, Hi, Wi, C, C, 3, (2, 2), 1)
    M, cp = Bn * geom.Ho * geom.Wo, ops.cpad(C, BF)
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    wf = _pack_fwd(w, cp).to(BF).cuda()
    y_nhwc = y.permute(0, 2, 3, 1)
    for f32 in (False, True):
        odt = torch.float32 if f32 else BF
        yd = torch.full((Bn, geom.Ho, geom.Wo, C), 7.0, dtype=odt, device="cuda")
        cs = torch.zeros(ops.gemm_num_mtiles(M, C, BF, gather=ops.GATHER_CONV_FWD), 2, C, dtype=torch.float32, device="cuda")
        ops.gemm(xd, wf, yd, dtype=BF, M=M, N=C, K=9 * cp, lda=C, ldb=9 * cp, ldc=C, gather=ops.GATHER_CONV_FWD, geom=geom,
                 Cpad=cp, colstats=cs, c_f32=f32)
        assert _last_kernel() == "gemm_halo_fs2_kernel<192" + (", f32>" if f32 else ">"), _last_kernel()
        assert torch.equal(yd.double().cpu(), y_nhwc.to(odt).double())
        assert torch.equal(cs[:, 0].double().sum(0).cpu(), y_nhwc.reshape(-1, C).sum(0))


# --------------------------------------------------------------------------------------------------------------------
# the fused dgrad of tests/test_gemm_gpu.py::test_conv_dgrad_fused_relu_bn_sums_exact at two image rows: every tile has
# one kernel row in the padding, the ReLU mask and the BatchNorm-backward sums come from the shortened accumulation
# --------------------------------------------------------------------------------------------------------------------
def _sparse_ints(shape, seed, p=0.25):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-1, 2, shape, generator=g) * (torch.rand(shape, generator=g) < p)).double()


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("nbn", [1, 2])
@pytest.mark.parametrize("with_res", [False, True])
def test_halo_dgrad_fused_relu_bn_sums_h2_exact(C, nbn, with_res):
    from htrvt_amd.engine import Engine, ModelShape
    ops = _ops()
    Bn, Hi, Wi = 2, 2, 256
    eng = Engine(ModelShape(80, (64, 512), 64, 2, 2), BF, "cuda")
    geom = ops.ConvGeom(Bn, Hi, Wi, C, C, 3, (1, 1), 1)
    # sparse +-1 operands keep |dx| far below 256, so the bf16 result and every float32 sum are exact integers
    w = _sparse_ints((C, C, 3, 3), 40)
    dy = _sparse_ints((Bn, C, Hi, Wi), 41)
    dx = torch.nn.grad.conv2d_input((Bn, C, Hi, Wi), w, dy, stride=(1, 1), padding=1).permute(0, 2, 3, 1)   # NHWC
    res = _ints((Bn, Hi, Wi, C), -3, 4, seed=42)
    relu_src = _ints((Bn, Hi, Wi, C), -1, 2, seed=43)
    g_ref = (dx + (res if with_res else 0.0)) * (relu_src > 0)
    assert g_ref.abs().max() < 256
    gen = torch.Generator().manual_seed(44)
    bnx = [_ints((Bn, Hi, Wi, C), -4, 5, seed=45 + t) for t in range(nbn)]
    mean = [torch.randint(-2, 3, (C,), generator=gen).double() for _ in range(nbn)]
    rstd = [torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)].double() for _ in range(nbn)]
    cp = ops.cpad(C, BF)
    wd = _pack_dgrad(w, cp).to(BF).cuda()
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    rows = eng.dgrad_tiles(geom)
    assert rows == Bn * Hi * Wi // 256
    parts = [torch.full((rows, 2, C), float("nan"), dtype=torch.float32, device="cuda") for _ in range(nbn)]
    bnb = [(bnx[t].to(BF).cuda(), mean[t].float().cuda(), rstd[t].float().cuda(), parts[t]) for t in range(nbn)]
    out = eng.conv_dgrad(dyd, wd, geom, residual=res.to(BF).cuda() if with_res else None, relu_src=relu_src.to(BF).cuda(), bnb=bnb)
    assert _last_kernel() == f"gemm_halo_kernel<{192 if C == 192 else 128}, true>", _last_kernel()
    assert torch.equal(out.double().cpu(), g_ref), float((out.double().cpu() - g_ref).abs().max())
    for t in range(nbn):
        xhat = (bnx[t] - mean[t]) * rstd[t]
        gg, xx = g_ref.reshape(-1, C), xhat.reshape(-1, C)
        want = torch.stack([torch.stack([gg[r0:r0 + 256].sum(0), (gg[r0:r0 + 256] * xx[r0:r0 + 256]).sum(0)])
                            for r0 in range(0, gg.shape[0], 256)])
        assert torch.equal(parts[t].double().cpu(), want), t


# --------------------------------------------------------------------------------------------------------------------
# weight gradients: float atomics and per-range slabs.  With kchunk = ceil(K / split / 64) * 64 pixels per range:
#   B*H*W = 2*2*256 = 1024: split 3 -> ranges of 384 (start mid-row), 7 -> 192, 8 -> 128; 16 -> 64: every range is ONE
#                           k-tile, and those in image row 0 (row 1) hold no live k-tile for kernel row 0 (row 2)
#   B*H*W = 3*4*512 = 6144: split 3 -> 2048 (whole rows), 7 -> 896 and 8 -> 768 (start mid-row); 32 -> 192: ranges
#                           [0, 192), [192, 384) lie inside image row 0
# kernels: 192 channels -> gemm_hwgrad16_kernel<96, 192> (layer 1), or two 64-channel units per workgroup on request
# (tile 18: the last workgroup's second unit is absent); 384 channels -> gemm_hwgrad_kernel<128, 192> (layers 2-3)
# --------------------------------------------------------------------------------------------------------------------
WGRAD_KERNELS = [(192, 0, "gemm_hwgrad16_kernel<96, 192>"), (192, 18, "gemm_hwgrad_kernel<128, 192, true>"),
                 (384, 0, "gemm_hwgrad_kernel<128, 192>")]
WGRAD_SHAPES = [  # B, Hi, Wi, stride, split factors
    (2, 2, 256, (1, 1), [3, 7, 8, 16]),
    (3, 4, 512, (1, 1), [3, 7, 8, 32]),
    (2, 1, 256, (1, 1), [3]),           # kernel rows 0 and 2 never read the image: their workgroups have nothing to add
    (2, 3, 256, (1, 1), [7]),
    (2, 8, 256, (1, 1), [7]),
    (2, 2, 256, (2, 1), [3]),           # row stride 2 (layer1.0.conv1): one output row
    (2, 16, 256, (2, 1), [7]),
]


@pytest.mark.parametrize("C,tile,kernel", WGRAD_KERNELS)
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]) + ("s2" if s[3][0] == 2 else ""))
def test_hwgrad_edge_rows_exact(shape, C, tile, kernel):
    ops = _ops()
    Bn, Hi, Wi, stride, splits = shape
    x, _, y, dy, _, gw = _reference(Bn, Hi, Wi, C, stride)
    geom = ops.ConvGeom(Bn, Hi, Wi, C, C, 3, stride, 1)
    K, cp = Bn * geom.Ho * geom.Wo, ops.cpad(C, BF)
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    want = _pack_fwd(gw, cp).permute(1, 2, 0)
    base = _ints((9, cp, C), -5, 6, seed=23)
    for split_k in splits:
        for slabs in (False, True):
            dwp = base.float().cuda()
            # slabs start as NaN: a range that skipped its slab instead of writing zeros would poison the sum
            ws = torch.full((split_k, 9 * cp, C), float("nan"), dtype=torch.float32, device="cuda") if slabs else None
            ops.gemm(xd, dyd, dwp, dtype=BF, M=9 * cp, N=C, K=K, lda=C, ldb=C, ldc=C, a_layout=ops.MNMAJOR, b_layout=ops.MNMAJOR,
                     gather=ops.GATHER_CONV_WGRAD, geom=geom, Cpad=cp, split_k=split_k, accumulate=True, c_f32=True, splitk_ws=ws,
                     tile=tile)
            assert _last_kernel() == kernel, _last_kernel()
            assert torch.equal(dwp.double().cpu(), base + want), (split_k, slabs)
