"""CPU-only checks of the host side: the C ABI library loads and exports every symbol
declared in include/htrvt.h, the drop-in module reproduces the reference's
construction (state_dict contract, seed-123 init bit for bit), refuses to run
without a GPU (no fallback), and the data-parallel gradient buckets reduce
correctly across two gloo ranks."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_exports_every_declared_symbol():
    import ctypes
    import htrvt_amd  # noqa: F401
    from htrvt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(htrvt_\w+)\s*\(", hdr))
    assert len(declared) >= 30
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} declared in include/htrvt.h but not exported"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
    assert set(_lib.PROTOTYPES) == declared
    assert _lib.lib.htrvt_version() >= 100


def test_ctypes_structures_match_the_header(tmp_path):
    """the ctypes mirrors of HtrvtGemmDesc / HtrvtRelayoutJob (htr-vt_amd/_lib.py) against the C compiler's layout of
    include/htrvt.h: size and the offset of every field"""
    import ctypes
    import subprocess
    import htrvt_amd  # noqa: F401
    from htrvt_amd import _lib
    structs = {"HtrvtGemmDesc": _lib.GemmDesc, "HtrvtRelayoutJob": _lib.RelayoutJob}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "htrvt.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_relayout_plan_is_host_side_and_refuses_malformed_jobs():
    """htrvt_relayout_plan (csrc/relayout.hip) only fills the workgroup ranges of a job table: callable without a GPU"""
    import ctypes
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import RelayoutJob, lib, RELAYOUT_PACK_CONV, RELAYOUT_CAST_TRANSPOSE, RELAYOUT_UNPACK_WGRAD

    def job(kind, d0, d1, taps=0, cpi=0, cpo=0, row_taps=0, tap0=0, dst0=8, dst1=8):
        j = RelayoutJob()
        j.src, j.dst0, j.dst1, j.kind, j.d0, j.d1 = 8, dst0, dst1, kind, d0, d1
        j.taps, j.cpad_in, j.cpad_out, j.row_taps, j.tap0 = taps, cpi, cpo, row_taps, tap0
        return j

    jobs = (RelayoutJob * 4)(job(RELAYOUT_PACK_CONV, 192, 64, 9, 64, 192, 9, 0),          # 6 x 2 tiles of 32 x 32
                             job(RELAYOUT_CAST_TRANSPOSE, 80, 768, cpi=80),                 # 12 x 2 tiles of 64 x 64
                             job(RELAYOUT_UNPACK_WGRAD, 40, 24, 9, 64, dst1=None),          # 2 x 1
                             job(RELAYOUT_PACK_CONV, 48, 24, 1, 64, 64, 10, 9, dst0=None))  # joint-pack slot 9 of 10: 2 x 1
    assert lib.htrvt_relayout_plan(jobs, 4) == 12 + 24 + 2 + 2
    assert [j.tile0 for j in jobs] == [0, 12, 36, 38] and [j.tiles_x for j in jobs] == [2, 12, 1, 1]
    for bad in (job(RELAYOUT_PACK_CONV, 48, 24, 9, 64, 64, 9, 1),           # tap slots 1 .. 9 of 9
                job(RELAYOUT_PACK_CONV, 48, 24, 10, 64, 64, 10, 0),         # more taps than a tile holds
                job(RELAYOUT_PACK_CONV, 48, 24, 9, 16, 64, 9, 0),           # padded row shorter than the channels
                job(RELAYOUT_CAST_TRANSPOSE, 80, 768, cpi=72),              # transposed rows shorter than the matrix
                job(RELAYOUT_UNPACK_WGRAD, 40, 24, 9, 64, dst0=None),       # nowhere to add the gradient
                job(7, 4, 4)):
        assert lib.htrvt_relayout_plan((RelayoutJob * 1)(bad), 1) < 0
    assert lib.htrvt_relayout_plan((RelayoutJob * 1)(jobs[0]), 0) < 0 and lib.htrvt_relayout_plan(None, 1) < 0


def test_create_model_matches_reference_init(golden_dir):
    from htrvt_amd.model import HTR_VT
    g = np.load(os.path.join(golden_dir, "create_model_init.npz"), allow_pickle=False)
    torch.manual_seed(123)
    m = HTR_VT.create_model(nb_cls=80, img_size=[64, 512])
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    abss = np.array([float(v.double().abs().sum()) for v in sd.values()])
    assert np.array_equal(sums, g["sums"]) and np.array_equal(abss, g["abssums"])   # same RNG stream, same bits
    assert sum(p.numel() for p in m.parameters()) == int(g["nparams"]) == 53486096
    assert m.embed_dim == 768 and m.num_patches == 128
    assert m._shape.blocks == [("full", None)] * 4
    assert len(m._shape.linears()) == 17 and m._shape.linears() == [n for n, mod in m.named_modules()
                                   if isinstance(mod, torch.nn.Linear) and (n.startswith("blocks.") or n == "head")]
    assert not m.pos_embed.requires_grad and m.mask_token.requires_grad
    with pytest.raises(TypeError):                     # duplicate kwargs fail exactly as in the reference
        HTR_VT.create_model(80, [64, 512], embed_dim=256)


def test_stem_block_table_matches_the_model():
    """ModelShape.stem_blocks() / stem_convs() against the modules of the v1 model at (64, 512)"""
    from htrvt_amd.model import HTR_VT
    m = HTR_VT.create_model(nb_cls=80, img_size=[64, 512])
    mods = dict(m.named_modules())
    convs = [(n, mod) for n, mod in mods.items() if isinstance(mod, torch.nn.Conv2d) and n.startswith("patch_embed.layer")]
    table = m._shape.stem_convs()
    assert [t[0] for t in table] == [n for n, _ in convs]
    for (name, Ci, Co, k, stride, pad), (_, mod) in zip(table, convs):
        assert (Ci, Co, k, stride, pad) == (mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride, mod.padding[0]), name
    blocks = m._shape.stem_blocks()
    assert len(blocks) == 6
    for b in blocks:
        assert b.downsample == (getattr(mods[b.prefix], "downsample", None) is not None), b.prefix
        assert (b.Cin, b.planes, b.stride) == (mods[b.prefix].conv1.in_channels, mods[b.prefix].conv1.out_channels, mods[b.prefix].conv1.stride)
    stem = [n for n, mod in mods.items() if isinstance(mod, torch.nn.Conv2d) and n.startswith("patch_embed.") and n != "patch_embed.conv1"]
    assert sorted(t[0] for t in table) == sorted(stem) and len(set(stem)) == len(stem) == 15


@pytest.mark.parametrize("Hi,Wi", [(5, 7), (4, 8)])
@pytest.mark.parametrize("k,stride,pad", [(3, (2, 2), 1), (3, (2, 1), 1), (3, (1, 1), 1), (1, (2, 2), 0)])
def test_conv_geom_parity_classes(k, stride, pad, Hi, Wi):
    import htrvt_amd  # noqa: F401
    from htrvt_amd.ops import ConvGeom
    g = ConvGeom(2, Hi, Wi, 8, 16, k, stride, pad)
    classes = list(g.parity_classes())
    assert [(a, b) for a, b, _, _, _ in classes] == [(a, b) for a in range(stride[0]) for b in range(stride[1])]
    assert sum(Hq * Wq for _, _, _, Hq, Wq in classes) == Hi * Wi
    assert sum(nt for _, _, nt, _, _ in classes) == k * k
    for a, b, nt, Hq, Wq in classes:
        assert nt == sum(1 for dy in range(k) for dx in range(k)
                         if (a + pad - dy) % stride[0] == 0 and (b + pad - dx) % stride[1] == 0)
        assert (Hq, Wq) == (len(range(a, Hi, stride[0])), len(range(b, Wi, stride[1])))
    if k == 1:
        assert [(a, b) for a, b, nt, _, _ in classes if nt] == [(0, 0)]


def test_no_cpu_fallback():
    from htrvt_amd.model import HTR_VT
    m = HTR_VT.create_model(nb_cls=80, img_size=[64, 512])
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 1, 64, 512))
    with pytest.raises(RuntimeError):
        m.patch_embed(torch.zeros(1, 1, 64, 512))      # sub-modules only own parameters


def test_span_mask_uses_reference_rng_stream(golden_dir):
    from htrvt_amd.model import HTR_VT
    g = np.load(os.path.join(golden_dir, "tiny_model.npz"), allow_pickle=False)
    m = HTR_VT.create_model(nb_cls=80, img_size=[64, 512])
    torch.manual_seed(11)
    keep = m.generate_span_mask(128, 0.4, 8)
    assert np.array_equal(keep.numpy(), g["keep_mask"])


def test_ema_deepcopy_and_state_dict_roundtrip():
    import copy
    from htrvt_amd.model import HTR_VT
    torch.manual_seed(0)
    m = HTR_VT.create_model(nb_cls=80, img_size=[64, 512])
    ema = copy.deepcopy(m)                               # utils.ModelEma (utils.py:130)
    assert ema._engines == {} and ema is not m
    sd = {("module." + k): v for k, v in m.state_dict().items()}
    stripped = {k[len("module."):]: v for k, v in sd.items()}   # test.py:30-40
    ema.load_state_dict(stripped, strict=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from htrvt_amd.model import HTR_VT
        from htrvt_amd.trainer import FlatParams
        torch.manual_seed(100 + rank)                     # ranks start DIFFERENT: broadcast must fix it
        m = HTR_VT.MaskedAutoencoderViT(80, img_size=[64, 512], patch_size=(4, 64), embed_dim=64, depth=2, num_heads=2,
                                        mlp_ratio=4, norm_layer=torch.nn.LayerNorm)
        fp = FlatParams(m, world_size=world)
        fp.check_views()
        # every rank holds rank-0's parameters now
        ref = fp.flat_p.clone()
        dist.broadcast(ref, 0)
        same_params = bool(torch.equal(ref, fp.flat_p))
        # gradients: rank r writes (r+1)/world * g0 (the 1/world factor is what the CTC kernel's grad_scale applies)
        g0 = torch.arange(fp.flat_g.numel(), dtype=torch.float32) % 97 - 48
        for n, g in fp.G.items():
            g.copy_((rank + 1) / world * torch.ones_like(g))
        fp.flat_g.mul_(g0)
        fp.reduce_encoder_bucket()
        fp.reduce_layer3_bucket()
        fp.reduce_stem_bucket()
        want = sum((r + 1) / world for r in range(world)) * g0
        pad_free = torch.zeros_like(want, dtype=torch.bool)
        for n, g in fp.G.items():
            off = (g.data_ptr() - fp.flat_g.data_ptr()) // 4
            pad_free[off:off + g.numel()] = True
        ok = bool(torch.allclose(fp.flat_g[pad_free], want[pad_free], rtol=1e-6, atol=1e-6))
        names = [n for n, _ in m.named_parameters() if _.requires_grad]
        first_enc = names.index("blocks.0.norm1.weight")
        enc_ok = all(n.startswith(("blocks.", "norm.", "head.")) for n in names[first_enc:]) and \
            not any(n.startswith(("blocks.", "norm.", "head.")) for n in names[:first_enc])
        l3_names = [n for n in names if n.startswith("patch_embed.layer3.")]
        l3_off = (fp.G[l3_names[0]].data_ptr() - fp.flat_g.data_ptr()) // 4
        enc_ok = enc_ok and 0 < fp.l3_start == l3_off < fp.enc_start and names.index(l3_names[-1]) == first_enc - 1
        out[rank] = (same_params, ok, enc_ok, int(fp.enc_start))
    finally:
        dist.destroy_process_group()


def test_dp_gradient_buckets_gloo_world2():
    world, port = 2, _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_dp_worker, args=(world, port, out), nprocs=world, join=True)
        res = dict(out)
    assert set(res) == {0, 1}
    for r in (0, 1):
        same_params, ok, enc_ok, enc_start = res[r]
        assert same_params and ok and enc_ok and enc_start > 0
    assert res[0][3] == res[1][3]


def test_no_kernel_runs_on_scratch():
    """a GEMM kernel that falls back to scratch memory (SGPR / VGPR spills past the register file) still computes the
    right numbers but runs several times slower: the layer-3 weight gradient once went from 0.63 to 2.76 ms that way.
    Allowed: the few-dword spills of the register-tight 12-wave variants (epilogue only, <= 32 bytes)."""
    import shutil
    import subprocess
    tool = os.path.join(ROOT, "tools", "check_kernels.sh")
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") and shutil.which("bash")):
        pytest.skip("ROCm llvm tools not available")
    out = subprocess.run(["bash", tool], capture_output=True, text=True, timeout=300).stdout
    worst = 0
    for line in out.splitlines():
        parts = line.split()
        if "scratch" in parts:
            worst = max(worst, int(parts[parts.index("scratch") + 1]))
    assert worst <= 32, out
