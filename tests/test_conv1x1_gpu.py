"""The streaming 1x1 downsample convolution (csrc/conv1x1.hip, behind htrvt_gemm with gather = CONV_FWD) kernel by kernel:
every instantiation conv1x1_fwd_kernel<KS, NWAVE> by name, column tails and leading dimensions, workgroups that walk
several 256-row tiles, and the launches the kernel declines.  Integer operands in [-2, 2] as in tests/test_gemm_gpu.py:
the bfloat16 output must equal F.conv2d in float64 (rounded once) bit for bit, and the float32 column sums are exact,
so they are compared PER TILE -- row t of colstats is the (sum, sum of squares) of output rows 256 t .. 256 t + 255."""
import pytest
import torch
import torch.nn.functional as F

from test_gemm_gpu import _ints, _pack_fwd

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _ops():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import ops
    return ops


def _last_kernel():
    from htrvt_amd._lib import lib
    return lib.htrvt_last_kernel().decode()


def _tile_sums(y):
    """y [M][N] float64 -> [ceil(M / 256)][2][N]; every sum is an integer below 2^24, so float32 holds it exactly"""
    M, N = y.shape
    T = (M + 255) // 256
    yp = torch.zeros(T * 256, N, dtype=torch.float64)
    yp[:M] = y
    yp = yp.view(T, 256, N)
    out = torch.stack([yp.sum(1), (yp * yp).sum(1)], dim=1)
    assert float(out.abs().max()) < 2 ** 24
    return out


class _Case:
    """one 1x1 convolution: operands on the device, the float64 reference [M][Co] on the host"""

    def __init__(self, Bn, Hi, Wi, Ci, Co, stride, lo=-2, hi=3, seed=10, cpad=0):
        ops = _ops()
        self.geom = ops.ConvGeom(Bn, Hi, Wi, Ci, Co, 1, stride, 0)
        self.M, self.N, self.cpad = Bn * self.geom.Ho * self.geom.Wo, Co, cpad or ops.cpad(Ci, BF)     # cpad: a wider weight row than the library's own padding
        x = _ints((Bn, Ci, Hi, Wi), lo, hi, seed=seed)
        w = _ints((Co, Ci, 1, 1), lo, hi, seed=seed + 1)
        self.ref = F.conv2d(x, w, None, stride=stride).permute(0, 2, 3, 1).reshape(self.M, Co)
        self.xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
        self.wd = _pack_fwd(w, self.cpad).to(BF).cuda()

    def run(self, colstats=True, ldc_extra=0, out_dtype=BF, **kw):
        """-> C [M][ldc] (sentinel 7 behind the N columns), colstats [tiles][2][N] or None, the kernel's name"""
        ops = _ops()
        ldc = self.N + ldc_extra
        c = torch.full((self.M, ldc), 7.0, dtype=out_dtype, device="cuda")
        cs = None
        if colstats:
            nmt = ops.gemm_num_mtiles(self.M, self.N, BF, gather=ops.GATHER_CONV_FWD)
            assert nmt == (self.M + 255) // 256
            cs = torch.full((nmt, 2, self.N), 99.0, dtype=torch.float32, device="cuda")
        ops.gemm(self.xd, self.wd, c, dtype=BF, M=self.M, N=self.N, K=self.cpad, lda=self.geom.Ci, ldb=self.cpad, ldc=ldc,
                 gather=ops.GATHER_CONV_FWD, geom=self.geom, Cpad=self.cpad, colstats=cs, **kw)
        return c, cs, _last_kernel()

    def kernel(self):
        return f"conv1x1_fwd_kernel<{self.cpad // 32}, {6 if self.N <= 192 else 12}>"

    def check(self, c, cs, name, served=True):
        """the route (unless a test forces one kernel family for every launch), the output bit for bit, padding columns
        untouched, column sums per tile"""
        if not getattr(_ops(), "_ENV_TILE", 0):
            assert (name == self.kernel()) if served else ("conv1x1_fwd_kernel" not in name), name
        assert torch.equal(c[:, :self.N].double().cpu(), self.ref.to(c.dtype).double())
        assert (c[:, self.N:] == 7).all()
        if cs is not None:
            assert torch.equal(cs.double().cpu(), _tile_sums(self.ref))


# B = 1, Ho = 3, Wo = 64: M = 192 (above the 128 rows below which the launch never reaches this kernel), a tail inside one tile;
# Wo = 64 is a whole number of stages at both stage widths (64 pixels up to Cpad = 192, 32 above).  Ci 72 / 200 / 320: the
# padded channels 72..127 / 200..255 / 320..383 must read as zeros (320 is a whole number of 64-channel k-tiles, so its
# weight rows are packed to 384 explicitly)
INSTANCES = [  # Bn, Hi, Wi, Ci, Co, stride, Cpad           -> KS, NWAVE
    (1, 6, 128, 64, 192, (2, 2), 64),        # 2, 6
    (1, 6, 128, 72, 192, (2, 2), 128),       # 4, 6
    (1, 6, 128, 192, 192, (2, 2), 192),      # 6, 6
    (1, 6, 128, 200, 192, (2, 2), 256),      # 8, 6
    (1, 6, 128, 320, 192, (2, 2), 384),      # 12, 6
    (1, 6, 128, 64, 384, (2, 2), 64),        # 2, 12
    (1, 6, 64, 128, 384, (2, 1), 128),       # 4, 12     column stride 1
    (3, 6, 128, 192, 384, (2, 2), 192),      # 6, 12     three images: M = 576, the third tile holds 64 rows
    (1, 6, 128, 256, 384, (2, 2), 256),      # 8, 12
    (1, 6, 128, 384, 384, (2, 2), 384),      # 12, 12
]


@pytest.mark.parametrize("cfg", INSTANCES)
def test_every_instantiation_by_name(cfg):
    case = _Case(*cfg[:6], cpad=cfg[6])
    assert case.M > 128 and case.geom.Wo == 64 and (cfg[6] == 384 or cfg[6] == _ops().cpad(cfg[3], BF))
    c, cs, name = case.run()
    case.check(c, cs, name)
    c2, _, name2 = case.run(colstats=False)
    case.check(c2, None, name2)
    assert torch.equal(c2, c)


def test_the_ten_cases_cover_the_ten_instantiations():
    got = {(cfg[6] // 32, 6 if cfg[4] <= 192 else 12) for cfg in INSTANCES}
    assert got == {(ks, nw) for ks in (2, 4, 6, 8, 12) for nw in (6, 12)}


@pytest.mark.parametrize("Ci,Co,ldc_extra", [(192, 200, 0),      # 12 waves, waves 7..11 own no column
                                              (64, 8, 0),         # one wave, one lane group of 8 columns
                                              (64, 768, 0),       # two column tiles
                                              (192, 200, 8),      # output rows inside a wider buffer
                                              (320, 8, 8)])
def test_column_tails_and_leading_dimensions(Ci, Co, ldc_extra):
    case = _Case(2, 6, 128, Ci, Co, (2, 2), cpad=384 if Ci == 320 else 0)
    c, cs, name = case.run(ldc_extra=ldc_extra)
    case.check(c, cs, name)


@pytest.mark.parametrize("Ci,Co,lo,hi", [(64, 1536, -2, 3),      # four column tiles, stages of 64 pixels (four per tile)
                                         (384, 768, -1, 2)])     # two column tiles, stages of 32 pixels (eight per tile)
def test_workgroups_that_walk_several_tiles(Ci, Co, lo, hi):
    """M = 256 (2 nwg + 1) + one stage, nwg = the workgroup count the host picks from the CU count: some workgroups walk
    three tiles and the others two, the last tile holds one stage; the ring carries DMA, counted waits and stores across
    the tile boundaries and the column sums are reset in between.  With and without colstats: the same output"""
    ops = _ops()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles_n = (Co + 383) // 384
    nwg = (2 if Co <= 192 else 1) * cus // tiles_n
    stage = 64 if ops.cpad(Ci, BF) <= 192 else 32
    M = 256 * (2 * nwg + 1) + stage
    rows = M // stage
    Bn = next((f for f in range(2, 64) if rows % f == 0), 1)        # several images where the row count allows it
    Ho = rows // Bn
    case = _Case(Bn, 2 * Ho, stage, Ci, Co, (2, 1), lo, hi)
    tiles_m = (M + 255) // 256
    print(f"\nconv1x1 multi-tile: {cus} CUs, N = {Co}: {tiles_n} column tiles, {nwg} workgroups each over {tiles_m} row tiles "
          f"(M = {M} = {Bn} x {Ho} x {stage})")
    assert case.M == M and tiles_m == 2 * nwg + 2 > nwg
    c, cs, name = case.run()
    case.check(c, cs, name)
    c2, _, name2 = case.run(colstats=False)
    assert name2 == name and torch.equal(c2, c)


def test_declined_launches_still_come_out_right():
    """an output row that is no whole number of stages, the eval-mode fold (column scale, bias, trailing ReLU: it stays on
    the GEMM kernels' epilogue) and a float32 output: another kernel serves the launch, and the result is exact"""
    case = _Case(2, 6, 96, 64, 192, (2, 2))                  # Wo = 48
    assert case.geom.Wo == 48 and case.M > 128
    c, cs, name = case.run()
    case.check(c, cs, name, served=False)

    case = _Case(2, 6, 128, 64, 192, (2, 2))                 # served as it is ...
    c, cs, name = case.run()
    case.check(c, cs, name)
    g = torch.Generator().manual_seed(6)                     # ... but not with the fold
    scale = torch.tensor([0.25, 0.5, 1.0, -0.5])[torch.randint(0, 4, (case.N,), generator=g)].double()
    bias = torch.randint(-8, 9, (case.N,), generator=g).double()
    raw = case.ref
    for kw, want in (({"bias": bias.float().cuda(), "colscale": scale.float().cuda(), "act": 3}, (raw * scale + bias).to(BF).double().clamp_min(0.0)),
                     ({"bias": bias.float().cuda(), "colscale": scale.float().cuda()}, raw * scale + bias),
                     ({"act": 3}, raw.clamp_min(0.0))):
        case.ref = want
        c, _, name = case.run(colstats=False, **kw)
        case.check(c, None, name, served=False)
    case.ref = raw
    c, _, name = case.run(colstats=False, out_dtype=torch.float32, c_f32=True)
    case.check(c, None, name, served=False)
