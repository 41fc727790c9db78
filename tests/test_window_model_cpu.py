"""Drop-in window-attention model (htrvt_amd.window.model.HTR_VT) on the CPU: the module tree, names, order and the
seed-123 initial state_dict of the reference fork (model_window/model/HTR_VT.py:233-276), pinned by
tests/golden/window_model.npz (tools/make_goldens_window.py ran the reference)."""
import os

import numpy as np
import pytest
import torch


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "window_model.npz"))


def test_window_state_dict_matches_reference_init(golden_dir):
    from htrvt_amd.window.model import HTR_VT as W
    g = _golden(golden_dir)
    torch.manual_seed(123)
    m = W.create_model(80, (64, 512))
    sd = m.state_dict()
    assert list(sd.keys()) == list(g["d768.keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["d768.shapes"])
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, g["d768.sums"], rtol=1e-6, atol=1e-6)
    assert "pos_embed" not in sd
    # the reference's zero-image pass through the stem, restated: every BatchNorm at running_var 0.9, one batch tracked
    for n, v in sd.items():
        if n.endswith("running_var"):
            assert torch.all(v == 0.9), n
        if n.endswith("num_batches_tracked"):
            assert int(v) == 1, n
    idx = sd["blocks.2.attn.relative_position_index"]
    assert idx.dtype == torch.int64 and idx.shape == (128, 128) and int(idx[0, 127]) == 254 and int(idx[127, 0]) == 0
    assert torch.all(sd["blocks.0.attn.relative_position_bias_table"] == 0)
    assert [(b.window_size, b.shift_size) for b in m.blocks] == [(16, 0), (16, 8), (0, 0), (0, 0)]
    assert m._shape.blocks == [("relpos", (16, 0)), ("relpos", (16, 8)), ("relpos", (0, 0)), ("relpos", (0, 0))]
    assert len(m._shape.linears()) == 17 and m._shape.linears() == [n for n, mod in m.named_modules()
                                   if isinstance(mod, torch.nn.Linear) and (n.startswith("blocks.") or n == "head")]


def test_model_shape_relpos_none_is_the_full_attention_block():
    from htrvt_amd.engine import ModelShape
    s = ModelShape(80, (64, 512), 768, 4, 6, pos_embed=False, whiten_logits=False, relpos=[(16, 0), None, (0, 0), None])
    assert s.blocks == [("relpos", (16, 0)), ("full", None), ("relpos", (0, 0)), ("full", None)]
    assert s.relpos == [(16, 0), None, (0, 0), None] and len(s.linears()) == 17


def test_window_create_model_rejects_unknown_kwargs():
    from htrvt_amd.window.model import HTR_VT as W
    with pytest.raises(TypeError):
        W.create_model(80, (64, 512), not_an_argument=1)
    with pytest.raises(NotImplementedError, match="split_bf16"):
        W.create_model(80, (64, 512), compute_dtype="split_bf16")


def test_window_model_refuses_cpu_tensors():
    from htrvt_amd.window.model import HTR_VT as W
    m = W.create_model(80, (64, 512)).eval()
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 1, 64, 512))
