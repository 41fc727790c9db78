"""The SGM forks' drop-in `model` package (htr-vt_amd/sgm/model) on the CPU: the head's module tree and seed-123 initial
state_dict and the vocabulary against tests/golden/sgm.npz (tools/make_goldens_sgm.py ran the reference), the fork layout
resolving through PYTHONPATH, model_sgm_2's encoder = the model_v1 drop-in's state_dict, and CPU tensors refused."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgm_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sgm.npz"))


def test_sgm_head_state_dict_matches_reference_init(golden_dir):
    from htrvt_amd.sgm.model.sgm_head import SGMHead
    g = _golden(golden_dir)
    torch.manual_seed(123)
    sd = SGMHead(768, 84).state_dict()
    assert list(sd.keys()) == list(g["init.keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["init.shapes"])
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, g["init.sums"], rtol=1e-6, atol=1e-6)


def test_sgm_head_strict_load_and_deepcopy():
    import copy
    from htrvt_amd.sgm.model.sgm_head import SGMHead
    torch.manual_seed(1)
    a = SGMHead(64, 20, d_txt=32, compute_dtype=torch.bfloat16)
    b = SGMHead(64, 20, d_txt=32)
    b.load_state_dict(a.state_dict(), strict=True)
    c = copy.deepcopy(a)
    assert c.compute_dtype == torch.bfloat16
    for (n, p), (_, q) in zip(a.named_parameters(), c.named_parameters()):
        assert torch.equal(p, q) and p.data_ptr() != q.data_ptr(), n
    with pytest.raises(TypeError):
        SGMHead(64, 20, compute_dtype=torch.float16)


def test_sgm_vocab_and_ids_match_reference(golden_dir):
    from htrvt_amd.sgm.model.sgm_head import build_sgm_vocab, texts_to_ids
    g = _golden(golden_dir)
    stoi, itos, pad, eos, bl, br = build_sgm_vocab(C.Converter())
    assert itos == list(g["vocab.itos"])
    assert (pad, eos, bl, br) == (80, 81, 82, 83) and all(stoi[c] == i for i, c in enumerate(itos))
    ids = texts_to_ids(["ab", ""], stoi)
    assert ids[0].dtype == torch.long and ids[0].tolist() == [stoi["a"], stoi["b"]] and ids[1].numel() == 0


def test_sgm_fork_layout_resolves_here():
    """`PYTHONPATH=<repo>/htr-vt_amd/sgm:<repo>` + the fork's imports, in a fresh interpreter"""
    code = ("import model, model.HTR_VT as H, model.sgm_head as S\n"
            "from model import HTR_VT\n"
            "from model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch\n"
            "print(H.__file__); print(S.__file__); print(HTR_VT.create_model.__module__)\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "htr-vt_amd", "sgm") + os.pathsep + ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split()
    want = os.path.join(ROOT, "htr-vt_amd", "sgm", "model")
    assert os.path.dirname(lines[0]) == want and os.path.dirname(lines[1]) == want, lines


def test_sgm_encoder_state_dict_is_model_v1s():
    from htrvt_amd.model import HTR_VT as V1
    from htrvt_amd.sgm.model import HTR_VT as M
    torch.manual_seed(123)
    a = V1.create_model(80, (64, 512)).state_dict()
    torch.manual_seed(123)
    m = M.create_model(80, (64, 512))
    b = m.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert isinstance(m, V1.MaskedAutoencoderViT) and hasattr(m, "forward_features")
    assert m._shape.blocks == [("full", None)] * 4
    assert len(m._shape.linears()) == 17 and m._shape.linears() == [n for n, mod in m.named_modules()
                                   if isinstance(mod, torch.nn.Linear) and (n.startswith("blocks.") or n == "head")]


def test_sgm_refuses_cpu_tensors():
    from htrvt_amd.sgm.model import HTR_VT as M
    from htrvt_amd.sgm.model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch
    stoi = build_sgm_vocab(C.Converter())[0]
    with pytest.raises(RuntimeError, match="MI355X"):
        make_context_batch(["abc"], stoi, device="cpu")
    head = SGMHead(64, 84, d_txt=32)
    ids = torch.zeros(1, 3, 5, dtype=torch.long)
    with pytest.raises(RuntimeError, match="MI355X"):
        head(torch.zeros(1, 8, 64), ids, ids, torch.zeros(1, 3, dtype=torch.long), torch.ones(1, 3))
    m = M.create_model(80, (64, 512)).eval()
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 1, 64, 512), return_features=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward_features(torch.zeros(1, 1, 64, 512))
