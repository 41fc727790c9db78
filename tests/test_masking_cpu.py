"""htrvt_amd.masking and the construction of the htrvt_amd.sgm_mms drop-in, on the CPU, against what the reference fork
model_sgm_mms_attach gave on the CPU (tests/golden/sgm_mms.npz, tools/make_goldens_sgm_mms.py): the generators bit for bit
after the same seeds, the random streams behind every call, no device round trips inside the block and span loops, the
drop-in's initial state_dict."""
import os
import random
from functools import partial

import numpy as np
import pytest
import torch

import sgm_mms_cases as C


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sgm_mms.npz"))


def _tiny_dropin(num_patches=1):
    from htrvt_amd.sgm_mms.model import HTR_VT as M
    return M.MaskedAutoencoderViT(80, img_size=[64, 64 * num_patches], patch_size=(4, 64), embed_dim=32, depth=1, num_heads=1,
                                  mlp_ratio=1, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def _call(kind, B, L, kw, model):
    """the drop-in's counterpart of the fork call the fixture recorded: bool [B, L], True = masked"""
    from htrvt_amd import masking
    kw = dict(kw)
    if kind == "random":
        return masking.mask_random_1d(B, L, kw["ratio"], "cpu")
    if kind == "block":
        return masking.mask_block_1d(B, L, kw["ratio"], "cpu", **({"min_block": kw["min_block"]} if "min_block" in kw else {}))
    if kind == "span":
        return masking.mask_span_1d(B, L, kw["ratio"], kw["max_span"], "cpu")
    if kind == "span_old":
        return masking.mask_span_old_1d(B, L, kw["ratio"], kw["max_span"], "cpu")
    ratios = kw.pop("mms_ratios", None)         # through the model: it honours mms_ratios as the fork does
    if ratios is not None:
        model.mms_ratios = ratios
    try:
        keep = model.generate_mms_mask(torch.zeros(B, L, 1), **kw)
    finally:
        if ratios is not None:
            del model.mms_ratios
    assert keep.shape == (B, L, 1) and keep.dtype == torch.float32 and set(keep.unique().tolist()) <= {0.0, 1.0}
    return keep[..., 0] == 0


def test_cases_cover_the_edges(golden):
    names = [c[0] for c in C.GEN_CASES]
    assert len(set(names)) == len(names)
    kinds = {c[1] for c in C.GEN_CASES}
    assert kinds == {"random", "block", "span", "span_old", "mms"}
    for kind in ("random", "block", "span", "mms"):
        assert {(B, L) for _, k, B, L, _ in C.GEN_CASES if k == kind} == set(C.SHAPES), kind
    span = [(L, kw["ratio"], kw["max_span"]) for _, k, _, L, kw in C.GEN_CASES if k == "span"]
    assert {r for _, r, _ in span} == {0.0, 0.004, 0.25, 0.4, 0.6, 0.8} and {s for _, _, s in span} == {1, 8, 300}
    assert all(s > L for L, _, s in span if s == 300)
    assert int(round(0.004 * 64)) == 0 and int(round(0.004 * 200)) == 1
    old = [int(L * kw["ratio"]) // max(1, kw["max_span"]) for _, k, _, L, kw in C.GEN_CASES if k == "span_old"]
    assert 0 in old and 1 in old and max(old) > 2
    # every recorded case ended before the fork's cap of 10 000 trials, and some block / span cases needed several
    trials = {n: int(golden[f"gen.{n}.trials"]) for n in names}
    assert max(trials.values()) < 10000 and max(trials.values()) > 100
    # a block case whose remaining target fell below min_block: more masked tokens than the target
    over = [n for n, k, B, L, kw in C.GEN_CASES if k == "block" and kw["ratio"] > 0
            and golden[f"gen.{n}.mask"].sum(1).max() > int(round(kw["ratio"] * L))]
    assert over


@pytest.mark.parametrize("index", range(len(C.GEN_CASES)), ids=[c[0] for c in C.GEN_CASES])
def test_generators_match_the_fork_bit_for_bit(golden, index):
    name, kind, B, L, kw = C.GEN_CASES[index]
    model = _tiny_dropin() if kind == "mms" else None
    random.seed(C.gen_seed(index))
    torch.manual_seed(C.gen_seed(index))
    mask = _call(kind, B, L, kw, model)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (B, L)
    assert np.array_equal(mask.numpy(), golden[f"gen.{name}.mask"])
    # the streams were consumed exactly as the fork consumes them
    assert random.random() == float(golden[f"gen.{name}.next_random"])
    assert np.array_equal(torch.rand(1).numpy(), golden[f"gen.{name}.next_torch"])


def test_model_helpers_delegate(golden):
    """the fork's method names on the drop-in give the fork's masks"""
    m = _tiny_dropin()
    calls = {"random": lambda B, L, kw: m._mask_random_1d(B, L, kw["ratio"], "cpu"),
             "block": lambda B, L, kw: m._mask_block_1d(B, L, kw["ratio"], "cpu"),
             "span": lambda B, L, kw: m._mask_span_1d(B, L, kw["ratio"], kw["max_span"], "cpu"),
             "span_old": lambda B, L, kw: m._mask_span_old_1d(B, L, kw["ratio"], kw["max_span"], "cpu")}
    done = set()
    for i, (name, kind, B, L, kw) in enumerate(C.GEN_CASES):
        if kind in calls and "min_block" not in kw and (B, L) == (4, 64) and kw["ratio"] in (0.3, 0.4):
            random.seed(C.gen_seed(i))
            torch.manual_seed(C.gen_seed(i))
            assert np.array_equal(calls[kind](B, L, kw).numpy(), golden[f"gen.{name}.mask"]), name
            done.add(kind)
    assert done == set(calls)
    # the legacy span mask (HTR_VT.py:349-357 of the fork): the CPU generator's draws, the same spans for every sample
    torch.manual_seed(5)
    keep = m.generate_span_mask(torch.zeros(3, 64, 8), 0.4, 8)
    torch.manual_seed(5)
    want = torch.ones(3, 64, 1)
    for _ in range(int(64 * 0.4) // 8):
        idx = torch.randint(64 - 8, (1,))
        want[:, idx:idx + 8, :] = 0
    assert torch.equal(keep, want)


def test_block_and_span_loops_make_no_tensor_round_trips(monkeypatch):
    """structural: inside the block / span loops nothing may read a tensor back (.item(), .cpu(), .tolist(), bool(), int()),
    on any device -- the bookkeeping is host memory and the tensor appears once, at the end"""
    from htrvt_amd import masking

    def forbidden(name):
        def f(self, *a, **k):
            raise AssertionError(f"Tensor.{name} called inside a mask generator")
        return f
    for name in ("item", "cpu", "tolist", "__bool__", "__int__", "__float__", "__index__", "numpy", "any", "sum"):
        monkeypatch.setattr(torch.Tensor, name, forbidden(name))
    created = []
    real_from_numpy = torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: created.append(a.shape) or real_from_numpy(a))
    random.seed(3)
    m1 = masking.mask_block_1d(4, 64, 0.4, "cpu")
    m2 = masking.mask_span_1d(4, 64, 0.4, 8, "cpu")
    m3 = masking.mask_span_1d(4, 64, 0.8, 300, "cpu")
    assert created == [(4, 64)] * 3                     # one tensor per call
    torch.manual_seed(3)
    keep = masking.generate_mms_mask(4, 64, "cpu", max_span_length=8)
    assert created == [(4, 64)] * 4                     # block and span united on the host: one upload
    monkeypatch.undo()
    assert m1.sum(1).min() >= 26 and m2.sum(1).min() >= 26 and m3.sum(1).min() >= 51 and keep.shape == (4, 64, 1)


def test_dropin_construction_matches_the_fork(golden):
    from htrvt_amd.sgm_mms.model import HTR_VT as M
    from htrvt_amd.sgm.model import HTR_VT as SGM
    torch.manual_seed(123)
    m = M.create_model(80, (64, 512))
    assert isinstance(m, SGM.MaskedAutoencoderViT)
    sd = m.state_dict()
    assert list(sd.keys()) == list(golden["init.keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(golden["init.shapes"])
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    assert np.array_equal(sums, golden["init.sums"])
    # the fork's interface
    import inspect
    assert list(inspect.signature(m.forward).parameters)[:6] == ["x", "use_masking", "return_features", "mask_mode", "mask_ratio",
                                                                  "max_span_length"]
    assert list(inspect.signature(m.forward_features).parameters)[:7] == ["x", "use_masking", "mask_mode", "mask_ratio",
                                                                           "max_span_length", "ratios", "block_params"]
    sig = inspect.signature(m.forward_features).parameters
    assert (sig["mask_mode"].default, sig["mask_ratio"].default, sig["max_span_length"].default) == ("mms", 0.5, 8)
    for helper in ("_mask_random_1d", "_mask_block_1d", "_mask_span_1d", "_mask_span_old_1d", "generate_mms_mask",
                   "generate_span_mask"):
        assert callable(getattr(m, helper))
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 1, 64, 512))
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward_features(torch.zeros(1, 1, 64, 512), use_masking=True, mask_mode="block", mask_ratio=0.4)


def test_dropin_package_layout():
    """`from model import HTR_VT`, `from model.sgm_head import ...` with htr-vt_amd/sgm_mms first on sys.path"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from model import HTR_VT, resnet18\n"
            "from model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch\n"
            "m = HTR_VT.create_model(80, (64, 512))\n"
            "assert type(m).__module__ == 'model.HTR_VT' and hasattr(m, '_mask_span_old_1d')\n"
            "print('ok')\n") % (os.path.join(root, "htr-vt_amd", "sgm_mms"), root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
