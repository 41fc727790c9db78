"""tests/svtr_refs.py against tests/golden/svtr.npz (arrays the fork's own MixingBlock / Merging / Combining produced in
float64, and its build_local_mask as bits), the box's geometry, the initial state_dict of htr-vt_amd/svtr.py against the
fork's, the refusals, and the new entry points' declarations.
No GPU: the package itself needs the built library to import, so svtr.py (and the swin.py it imports from) is loaded on a stub
of its imports."""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import svtr_cases as C
import svtr_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = ("htrvt_attn_nbr2d_supported", "htrvt_attn_nbr2d_fwd", "htrvt_attn_nbr2d_bwd")
SEQ_OPS = ("nbr2d_attention_fwd", "nbr2d_attention_bwd", "mixing_block_fwd", "mixing_block_bwd", "svtr_merge_fwd",
           "svtr_merge_bwd", "combining_fwd", "combining_bwd")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "svtr.npz"))


def rel(a, b):
    b = torch.as_tensor(b, dtype=F64)
    return float((a.double() - b).abs().max() / b.abs().max())


def load_svtr_module():
    """htr-vt_amd/svtr.py with its package imports stubbed: the module tree needs torch only"""
    names = ("_svtr_stub", "_svtr_stub.seq_ops", "_svtr_stub.swin", "_svtr_stub.svtr")
    saved = {k: sys.modules.get(k) for k in names}
    pkg = types.ModuleType("_svtr_stub")
    pkg.__path__ = []
    seq = types.ModuleType("_svtr_stub.seq_ops")
    seq.convert = None
    sys.modules["_svtr_stub"], sys.modules["_svtr_stub.seq_ops"] = pkg, seq
    pkg.seq_ops = seq
    try:
        for name in ("swin", "svtr"):
            spec = importlib.util.spec_from_file_location("_svtr_stub." + name, os.path.join(ROOT, "htr-vt_amd", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules["_svtr_stub." + name] = mod
            spec.loader.exec_module(mod)
            setattr(pkg, name, mod)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@pytest.fixture(scope="module")
def svtr():
    return load_svtr_module()


# ====================================================================== the restatement against the fork
@pytest.mark.parametrize("case", list(C.CASES))
def test_refs_reproduce_the_fork(gold, svtr, case):
    B, H, W, _, _ = C.CASES[case]
    x, dy = C.inputs(case)
    assert abs(float(x.double().sum()) - float(gold[f"{case}.xsum"])) < 1e-9      # the seeded inputs are the fixture's
    assert abs(float(dy.double().sum()) - float(gold[f"{case}.dysum"])) < 1e-9
    mods = C.case_modules(svtr, case)
    for tag, _, _, m in mods:            # rebuilt from their seeds: the modules the fixture's numbers come from
        for k, v in m.state_dict().items():
            assert abs(float(v.double().sum()) - float(gold[f"{case}.sums.{tag}.{k}"])) <= C.SUM_TOL * v.numel(), (tag, k)
    stages = [(tag, kind, args, m.state_dict()) for tag, kind, args, m in mods]
    y, dx, grads = R.case_grads(stages, x, dy, H, W)
    assert tuple(y.shape) == C.out_shape(case)
    assert rel(y, gold[f"{case}.y"]) < 1e-10 and rel(dx, gold[f"{case}.dx"]) < 1e-10
    seen = 0
    for name, g in grads.items():
        key = f"{case}.grad.{name}"
        if g.numel() > C.PROBE_ABOVE:
            p = C.probe(g)
            assert rel(p["gv"], gold[key + ".gv"]) < 1e-10 and rel(p["ug"], gold[key + ".ug"]) < 1e-10, name
            assert rel(p["max"], gold[key + ".max"]) < 1e-10, name
            seen += 3
        else:
            assert rel(g, gold[key]) < 1e-10, name
            seen += 1
    assert seen == sum(k.startswith(case + ".grad.") for k in gold.files)


def test_box_is_the_forks_mask(gold):
    """index arithmetic against the fork's build_local_mask, recorded as bits for seven map and box sizes"""
    keys = [k for k in gold.files if k.startswith("mask.")]
    assert len(keys) == 7
    for key in keys:
        (H, W), (kh, kw) = [tuple(map(int, part.split("x"))) for part in key.split(".")[1:]]
        N = H * W
        ref = torch.from_numpy(np.unpackbits(gold[key])[:N * N].reshape(N, N).astype(bool))
        assert torch.equal(R.visible(H, W, (kh, kw)), ref), key


def test_box_geometry():
    vis = R.visible(16, 24, (7, 11))
    count = vis.sum(1)
    assert int(count.min()) == 24 and int(count.max()) == 77
    assert int(count.view(16, 24)[0, 0]) == 24 and int(count.view(16, 24)[8, 12]) == 77
    for _, H, W, _, _, kh, kw in C.KERNEL_SHAPES:
        vis = R.visible(H, W, (kh, kw))
        assert torch.equal(vis, vis.t())                     # symmetric: the queries that see a key are the key's own box
        assert bool(vis.diagonal().all())
        if H <= kh // 2 + 1 and W <= kw // 2 + 1:
            assert bool(vis.all())
    for H, W, k in ((4, 6, (7, 11)), (1, 1, (7, 11)), (2, 3, (3, 5))):
        assert H <= k[0] // 2 + 1 and W <= k[1] // 2 + 1 and bool((R.visible(H, W, k).sum(1) == H * W).all())


@pytest.mark.parametrize("shape", [s for s in C.KERNEL_SHAPES if s[0] * s[1] * s[2] <= 1000], ids=lambda s: "x".join(map(str, s)))
def test_box_form_is_the_dense_masked_form(shape):
    """the reference's per-offset form against the fork's form, dense scores with -inf outside the box"""
    B, H, W, heads, hd, kh, kw = shape
    qkv, _ = C.kernel_inputs(shape, F64)
    a = R.nbr2d_attention(qkv, B, H, W, heads, (kh, kw))
    b = R.dense_attention(qkv, B, H * W, heads, R.visible(H, W, (kh, kw)))
    assert float((a - b).abs().max()) < 1e-12


# ====================================================================== the modules' trees
def test_module_trees_and_seeded_inits_are_the_forks(gold, svtr):
    for tag, (kind, args, kwargs) in C.INIT.items():
        torch.manual_seed(C.INIT_SEED)
        mod = C.build(svtr, kind, args, kwargs)
        sd = mod.state_dict()
        assert list(sd.keys()) == list(gold[f"init.{tag}.keys"])
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(gold[f"init.{tag}.shapes"])
        for (k, v), ref in zip(sd.items(), gold[f"init.{tag}.sums"]):
            assert float(v.double().sum()) == float(ref), k
        assert not list(mod.buffers())
        torch.manual_seed(C.INIT_SEED)
        sd = C.perturb(C.build(svtr, kind, args, kwargs)).state_dict()
        pre = f"sd.{tag}."
        for k, v in sd.items():      # the perturbed seed-123 module IS the fixture's module, value for value
            assert torch.equal(v, torch.from_numpy(gold[pre + k])), k
        m = C.build(svtr, kind, args, kwargs)        # a fork checkpoint's entries load strictly
        m.load_state_dict({k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)}, strict=True)
    blk = C.build(svtr, *C.INIT["block"])
    assert list(blk.state_dict().keys()) == [
        "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
        "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"]
    assert [n for n, _ in blk.named_children()] == ["norm1", "attn", "norm2", "mlp"]
    assert [n for n, _ in blk.attn.named_children()] == ["qkv", "proj"]
    assert blk.attn.local is True and tuple(blk.attn.local_k) == (7, 11) and blk.attn.num_heads == 1
    assert blk.attn.head_dim == 32 and blk.attn.scale == 32 ** -0.5 and blk.attn.qkv.bias is None
    attn = C.build(svtr, *C.INIT["attn"])
    assert tuple(attn.local_k) == (3, 5) and list(attn.state_dict().keys()) == ["qkv.weight", "proj.weight", "proj.bias"]
    assert svtr.MultiHeadSelfAttention(256).local is False and svtr.MultiHeadSelfAttention(256).num_heads == 8
    mrg = C.build(svtr, *C.INIT["merge"])
    assert list(mrg.state_dict().keys()) == ["conv.weight", "conv.bias", "norm.weight", "norm.bias"]
    assert [n for n, _ in mrg.named_children()] == ["conv", "norm"] and tuple(mrg.conv.weight.shape) == (32, 16, 3, 3)
    assert list(C.build(svtr, *C.INIT["comb"]).state_dict().keys()) == ["fc.weight", "fc.bias"]
    assert [n for n, _ in svtr.Combining(64, 64).named_children()] == ["fc", "act", "drop"]


def test_refusals(svtr):
    ctors = {"attn": lambda **k: svtr.MultiHeadSelfAttention(64, 2, local=True, **k),
             "global": lambda **k: svtr.MultiHeadSelfAttention(64, 2, **k),
             "block": lambda **k: svtr.MixingBlock(64, 2, local=True, **k),
             "merge": lambda **k: svtr.Merging(64, 128, **k),
             "comb": lambda **k: svtr.Combining(64, 64, **k)}
    for tag, ctor in ctors.items():
        with pytest.raises(TypeError):
            ctor(compute_dtype=torch.float16)
        m = ctor().eval()
        x = torch.zeros(2, 32, 64)
        with pytest.raises(RuntimeError, match="runs on an MI355X only: move the module and its input to cuda"):
            m(x, 4, 8)
        with pytest.raises(ValueError):              # N != H * W: the fork's fallback branch is not reproduced
            m(x, 4, 16)
        with pytest.raises(ValueError):
            m(torch.zeros(2, 32, 48), 4, 8)
    for ctor in (svtr.MultiHeadSelfAttention, svtr.MixingBlock):
        with pytest.raises(ValueError):              # dim % num_heads
            ctor(100, 3)
        for dim, heads in ((32, 2), (96, 2), (256, 2), (64, 8)):      # head widths 16, 48, 128, 8
            with pytest.raises(ValueError):
                ctor(dim, heads)
        assert ctor(128, 2).attn.head_dim == 64 if ctor is svtr.MixingBlock else ctor(128, 2).head_dim == 64
    for local_k in ((6, 11), (7, 10), (9, 11), (7, 13), (0, 11), (7, -1)):
        with pytest.raises(ValueError):
            svtr.MultiHeadSelfAttention(64, 2, local=True, local_k=local_k)
    for local_k in ((1, 1), (3, 5), (7, 11), (1, 11), (7, 1)):
        svtr.MultiHeadSelfAttention(64, 2, local=True, local_k=local_k)
    with pytest.raises(NotImplementedError):
        svtr.Combining(64, 64).train()(torch.zeros(1, 32, 64), 4, 8)         # the constructor's default drop=0.1


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    src = open(os.path.join(ROOT, "htr-vt_amd", "_lib.py")).read()
    seq = open(os.path.join(ROOT, "htr-vt_amd", "seq_ops.py")).read()
    var = open(os.path.join(ROOT, "htr-vt_amd", "variants.py")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", hdr), f"{name} is not declared in include/htrvt.h"
        assert f'"{name}"' in src, f"{name} has no ctypes prototype"
    for name in SEQ_OPS:
        assert f"def {name}(" in seq, name
    assert "def nbr2d_attention_fwd(qkv, B, H, W, h, kernel, save=True)" in seq
    assert "def nbr2d_attention_bwd(qkv, out, dout, lse, B, H, W, h, kernel)" in seq
    assert "def neighborhood_attention_2d(qkv, B, H, W, heads, kernel=(7, 11))" in var
    assert "def nbr2d_supported(head_dim, kernel, dtype)" in var
    assert os.path.exists(os.path.join(ROOT, "htr-vt_amd", "csrc", "svtr.hip"))
