"""Drop-in LGP model (htrvt_amd.lgp.model.HTR_VT) on the CPU: the module tree, names, order and the seed-123 initial
state_dict of the reference fork (model_lgp/model/HTR_VT.py:152-276, plg.py), pinned by tests/golden/lgp_model.npz
(tools/make_goldens_lgp.py ran the reference)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lgp_model.npz"))


def test_lgp_state_dict_matches_reference_init(golden_dir):
    from htrvt_amd.lgp.model import HTR_VT as L
    g = _golden(golden_dir)
    torch.manual_seed(123)
    m = L.create_model(80, (64, 512))
    sd = m.state_dict()
    assert len(sd) == 177 and sum(p.numel() for p in m.parameters()) == 67558932
    assert list(sd.keys()) == list(g["d768.keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["d768.shapes"])
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, g["d768.sums"], rtol=1e-6, atol=1e-6)
    # pos_embed: a non-persistent buffer as in the fork -- callers find it on the model, checkpoints do not carry it
    assert "pos_embed" not in sd
    assert m.pos_embed.shape == (1, 128, 768) and m.pos_embed.dtype == torch.float32
    assert [n for n, _ in m.named_buffers() if "patch_embed" not in n] == ["pos_embed"]
    a = sd["blocks.3.global_attn.logit_alpha"]
    assert a.dim() == 0 and abs(float(a) - float(np.log(0.4 / 0.6))) < 1e-6
    assert m.blocks[0].global_attn.branch_norm.eps == 1e-5 and m.blocks[0].norm1.eps == 1e-6
    assert m._shape.lgp == (12, 64, 1e-5) and m._shape.num_patches == 128
    assert m._shape.blocks == [("lgp", (12, 64, 1e-5))] * 4
    assert len(m._shape.linears()) == 29 and m._shape.linears() == [n for n, mod in m.named_modules()
                                   if isinstance(mod, torch.nn.Linear) and (n.startswith("blocks.") or n == "head")]
    assert m._shape.linears()[:7] == ["blocks.0." + n for n in ("local_attn.qkv", "local_attn.proj", "global_attn.qkv",
                                                                 "global_attn.proj", "fuse", "mlp.fc1", "mlp.fc2")]


def test_lgp_pos_embed_is_the_grid_of_the_real_token_count():
    from htrvt_amd.lgp.model import HTR_VT as L
    m = L.MaskedAutoencoderViT(80, img_size=[64, 800], patch_size=(4, 64), embed_dim=256, depth=1, num_heads=4)
    assert m.tokens == 200 and m.num_patches == 16 * 12          # the fork's own estimate is kept, the stem's count is used
    pe = m.pos_embed[0]
    assert pe.shape == (200, 256)
    omega = 1.0 / 10000 ** (np.arange(64) / 64.0)
    np.testing.assert_allclose(pe[:, :64].numpy(), np.sin(np.arange(200)[:, None] * omega), atol=1e-6)
    assert torch.all(pe[:, 128:192] == 0) and torch.all(pe[:, 192:] == 1)      # H' = 1: sin(0), cos(0)


def test_lgp_fork_layout_import():
    """the fork's scripts run with htr-vt_amd/lgp and the repository root in front of sys.path"""
    code = ("from model import HTR_VT; from model.plg import LocalGlobalParallelBlockSimple as B, WindowMHSA1D, PooledGlobalMHSA;"
            "import model.resnet18; m = HTR_VT.create_model(nb_cls=80, img_size=[64, 512]);"
            "assert type(m.blocks[0]) is B and type(m.blocks[0].local_attn) is WindowMHSA1D;"
            "assert HTR_VT.Attention and HTR_VT.Block; print('ok', HTR_VT.__file__)")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "htr-vt_amd", "lgp"), ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert out.returncode == 0, out.stderr
    assert os.path.join("htr-vt_amd", "lgp", "model", "HTR_VT.py") in out.stdout


def test_lgp_refusals():
    from htrvt_amd.lgp.model import HTR_VT as L
    from htrvt_amd.lgp.model import plg
    with pytest.raises(TypeError):
        L.create_model(80, (64, 512), not_an_argument=1)
    with pytest.raises(NotImplementedError, match="split_bf16"):
        L.create_model(80, (64, 512), compute_dtype="split_bf16")
    with pytest.raises(NotImplementedError, match="64-pixel"):      # the position table is the fork's for a stem grid [1, N] only
        L.create_model(80, (128, 512))
    with pytest.raises(NotImplementedError, match="pool='max'"):
        plg.LocalGlobalParallelBlockSimple(256, 4, pool='max')
    with pytest.raises(NotImplementedError, match="pool='max'"):
        plg.PooledGlobalMHSA(256, 4, pool='max')
    with pytest.raises(TypeError):
        plg.LocalGlobalParallelBlockSimple(256, 4, not_an_argument=1)
    with pytest.raises(RuntimeError, match="only owns parameters"):
        plg.LocalGlobalParallelBlockSimple(256, 4)(torch.zeros(1, 24, 256))


def test_lgp_model_refuses_cpu_tensors():
    from htrvt_amd.lgp.model import HTR_VT as L
    m = L.create_model(80, (64, 512)).eval()
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 1, 64, 512))
