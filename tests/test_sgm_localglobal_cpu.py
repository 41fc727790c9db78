"""Drop-in SGM local-global model (htrvt_amd.sgm_localglobal.model.HTR_VT) on the CPU: both import routes, the module tree
and seed-123 initial state_dict of the reference fork (model_sgm_localglobal/model/HTR_VT.py), pinned by
tests/golden/sgm_localglobal.npz (tools/make_goldens_sgm_localglobal.py ran the reference); the block kinds the engine is
given, the classes the fork defines but never builds, ModelShape's refusals and the ABI of the shifted window kernel."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgm_localglobal_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("htrvt_attn_local_shift_supported", "htrvt_attn_local_shift_fwd", "htrvt_attn_local_shift_bwd")


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sgm_localglobal.npz"))


def test_slg_state_dict_matches_reference_init(golden_dir):
    from htrvt_amd.sgm_localglobal.model import HTR_VT as M
    g = _golden(golden_dir)
    torch.manual_seed(123)
    m = M.create_model(80, (64, 512))
    sd = m.state_dict()
    assert list(sd.keys()) == list(g["d768.keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["d768.shapes"])
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, g["d768.sums"], rtol=1e-6, atol=1e-6)
    pe = dict(m.named_parameters())["pos_embed"]
    assert isinstance(m.pos_embed, torch.nn.Parameter) and not pe.requires_grad and pe.shape == (1, 128, 768)
    assert m.compute_dtype == torch.float32


def test_slg_block_kinds_and_shape():
    from htrvt_amd.sgm_localglobal.model import HTR_VT as M
    m = M.create_model(80, (64, 512))
    assert m.block_kinds() == SC.KINDS == m._shape.local == [(12, 0), (12, 6), None, None]
    assert [type(b) for b in m.blocks] == [M.LocalBlock1D, M.LocalBlock1D, M.Block, M.Block]
    assert type(m.blocks[1].attn) is M.WindowMHSA1D and type(m.blocks[2].attn) is M.Attention
    assert (m.blocks[0].attn.shift, m.blocks[1].attn.shift, m.blocks[1].attn.win) == (0, 6, 12)
    assert m._shape.relpos is None and m._shape.lgp is None and m._shape.num_patches == 128
    assert m._shape.blocks == [("local", (12, 0)), ("local", (12, 6)), ("full", None), ("full", None)]
    assert len(m._shape.linears()) == 17 and m._shape.linears() == [n for n, mod in m.named_modules()
                                   if isinstance(mod, torch.nn.Linear) and (n.startswith("blocks.") or n == "head")]
    assert m._shape.linears()[:4] == ["blocks.0." + n for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]
    for W, patch in SC.TINY.items():        # the tiny geometries of the fixture: the table has as many rows as the stem leaves
        t = M.MaskedAutoencoderViT(SC.NB_CLS, img_size=[64, W], patch_size=patch, **SC.TINY_KW)
        assert t.num_patches == W // 4 == t._shape.num_patches and t.block_kinds() == SC.KINDS


def test_slg_fork_layout_import():
    """the fork's scripts run with htr-vt_amd/sgm_localglobal and the repository root in front of sys.path"""
    code = ("from model import HTR_VT; from model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch;"
            "import model.resnet18; import htrvt_amd.sgm.model.sgm_head as H; assert SGMHead is H.SGMHead;"
            "m = HTR_VT.create_model(nb_cls=80, img_size=[64, 512]);"
            "assert type(m.blocks[1]) is HTR_VT.LocalBlock1D and type(m.patch_embed) is model.resnet18.ResNet18;"
            "print('ok', HTR_VT.__file__)")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "htr-vt_amd", "sgm_localglobal"), ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert out.returncode == 0, out.stderr
    assert os.path.join("htr-vt_amd", "sgm_localglobal", "model", "HTR_VT.py") in out.stdout
    from htrvt_amd.sgm_localglobal.model import HTR_VT, resnet18, sgm_head      # the package route
    from htrvt_amd.model.resnet18 import ResNet18
    assert resnet18.ResNet18 is ResNet18 and sgm_head.SGMHead.__module__.endswith("sgm.model.sgm_head")
    assert HTR_VT.create_model


def test_slg_unbuilt_classes_construct_and_refuse_forward():
    from htrvt_amd.sgm_localglobal.model import HTR_VT as M
    built = [M.PooledGlobalMHSA(256, 4), M.LocalGlobalParallelBlock(256, 4, 12), M.GlobalPooledBlock(256, 4),
             M.LayerScale(256)]
    assert [n for n, _ in built[1].named_parameters()][:4] == ["norm1.weight", "norm1.bias", "local_attn.qkv.weight",
                                                               "local_attn.qkv.bias"]
    assert "fuse.weight" in dict(built[1].named_parameters()) and built[3].gamma.shape == (256,)
    assert built[0].norm.elementwise_affine is False
    for mod in built + [M.WindowMHSA1D(256, 4, 12, shift=6), M.LocalBlock1D(256, 4, 12, shift=True), M.Block(256, 4, 64),
                        M.Attention(256, 64)]:
        with pytest.raises(RuntimeError, match="only owns parameters"):
            mod(torch.zeros(1, 12, 256))


def test_slg_refusals():
    from htrvt_amd.sgm_localglobal.model import HTR_VT as M
    with pytest.raises(TypeError):
        M.create_model(80, (64, 512), not_an_argument=1)
    with pytest.raises(NotImplementedError, match="split_bf16"):
        M.create_model(80, (64, 512), compute_dtype="split_bf16")
    with pytest.raises(NotImplementedError, match="64-pixel"):
        M.create_model(80, (128, 512))
    with pytest.raises(ValueError, match="192 rows.*200 tokens"):      # the fork fails at x + pos_embed for this width
        M.create_model(80, (64, 800))
    with pytest.raises(NotImplementedError, match="dropout"):
        M.LocalBlock1D(256, 4, 12, drop=0.1)
    m = M.create_model(80, (64, 512))
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 1, 64, 512), return_features=True)


def test_model_shape_refuses_local_with_relpos_or_lgp():
    from htrvt_amd.engine import ModelShape
    kinds = [(12, 0), (12, 6), None, None]
    s = ModelShape(80, (64, 512), 768, 4, 6, local=kinds)
    assert s.local == kinds and s.num_patches == 128
    with pytest.raises(ValueError, match="local"):
        ModelShape(80, (64, 512), 768, 4, 6, local=kinds, relpos=[(12, 0)] * 4)
    with pytest.raises(ValueError, match="local"):
        ModelShape(80, (64, 512), 768, 4, 6, local=kinds, lgp=(12, 64, 1e-5), pos_table=torch.zeros(128, 768))
    with pytest.raises(AssertionError):
        ModelShape(80, (64, 512), 768, 4, 6, local=[(12, 12), None, None, None])       # shift < window
    with pytest.raises(AssertionError):
        ModelShape(80, (64, 512), 768, 4, 6, local=kinds[:3])


def test_shift_abi_is_declared_and_exported():
    from htrvt_amd import _lib
    header = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.PROTOTYPES
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), sym), ctypes.c_void_p).value       # the built library exports it
    assert re.search(r"htrvt_attn_local_shift_fwd\([^;]*int window,\s*int shift, float scale", header)
