"""tests/swin_refs.py against tests/golden/swin.npz (arrays the fork's own SwinBlock2D / HeightOnlyPatchMerging / Combining
produced in float64), the additive -100 mask against -inf, the initial state_dict of htr-vt_amd/swin.py against the fork's,
the refusals, and the new entry points' declarations.
No GPU: the package itself needs the built library to import, so swin.py is loaded on a stub of its imports."""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import swin_cases as C
import swin_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = ("htrvt_attn_win2d_supported", "htrvt_attn_win2d_fwd", "htrvt_attn_win2d_rows", "htrvt_attn_win2d_bwd")
SEQ_OPS = ("win2d_attention_fwd", "win2d_attention_bwd", "swin_block_fwd", "swin_block_bwd", "patch_merge_fwd", "patch_merge_bwd",
           "combining_fwd", "combining_bwd")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "swin.npz"))


def rel(a, b, scale=None):
    b = torch.as_tensor(b, dtype=F64)
    return float((a.double() - b).abs().max() / (b.abs().max() if scale is None else scale))


def load_swin_module():
    """htr-vt_amd/swin.py with its package imports stubbed: the module tree needs torch only"""
    pkg = types.ModuleType("_swin_stub")
    pkg.__path__ = []
    saved = {k: sys.modules.get(k) for k in ("_swin_stub", "_swin_stub.seq_ops")}
    seq = types.ModuleType("_swin_stub.seq_ops")
    seq.convert = None
    sys.modules["_swin_stub"], sys.modules["_swin_stub.seq_ops"] = pkg, seq
    pkg.seq_ops = seq
    try:
        spec = importlib.util.spec_from_file_location("_swin_stub.swin", os.path.join(ROOT, "htr-vt_amd", "swin.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@pytest.fixture(scope="module")
def swin():
    return load_swin_module()


def check_case_modules(gold, case, mods):
    """the modules rebuilt from their seeds are the ones the fixture's numbers come from"""
    for tag, _, _, m in mods:
        for k, v in m.state_dict().items():
            assert abs(float(v.double().sum()) - float(gold[f"{case}.sums.{tag}.{k}"])) <= C.SUM_TOL * v.numel(), (tag, k)


# ====================================================================== the restatement against the fork
@pytest.mark.parametrize("case", list(C.CASES))
def test_refs_reproduce_the_fork(gold, swin, case):
    B, H, W, _, _ = C.CASES[case]
    x, dy = C.inputs(case)
    assert torch.equal(x, torch.from_numpy(gold[f"{case}.x"])) and torch.equal(dy, torch.from_numpy(gold[f"{case}.dy"]))
    mods = C.case_modules(swin, case)
    check_case_modules(gold, case, mods)
    stages = [(tag, kind, args, m.state_dict()) for tag, kind, args, m in mods]
    y, dx, grads = R.case_grads(stages, x, dy, H, W)
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


def test_refs_roll_and_partition_are_torchs(swin):
    """the slot -> token arithmetic alone, against torch.roll + window_partition / window_reverse on every kernel shape, and
    the regions against their definition on the shifted coordinates.  (Which pairs the fork masks is pinned by the goldens:
    the 'block' case has four regions, the chain two.)"""
    for B, H, W, heads, hd, wh, ww, sh, sw in C.KERNEL_SHAPES:
        tok, reg = R.window_slots(H, W, (wh, ww), (sh, sw))
        ids = torch.arange(H * W, dtype=torch.float32).view(1, H, W, 1)
        rolled = torch.roll(ids, shifts=(-sh, -sw), dims=(1, 2))
        assert torch.equal(swin.window_partition(rolled, wh, ww).squeeze(-1).long(), tok)
        back = torch.roll(swin.window_reverse(swin.window_partition(rolled, wh, ww), wh, ww, H, W, 1), (sh, sw), (1, 2))
        assert torch.equal(back, ids)
        hs, ws = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
        regions = ((hs >= H - sh) & (sh > 0)).float() + 2 * ((ws >= W - sw) & (sw > 0)).float()
        assert torch.equal(swin.window_partition(regions.view(1, H, W, 1), wh, ww).squeeze(-1).long(), reg)


def test_additive_mask_differs_from_minus_infinity_only_at_large_scores():
    """at ordinary input scales -100 and -inf agree to the last bit, so only the pinned case can tell them apart; there the
    masked keys keep more than 0.99 of each row of the first region"""
    shape = (2, 8, 16, 2, 32, 4, 8, 2, 4)
    B, H, W, heads, hd, wh, ww, sh, sw = shape
    qkv, table, _ = [t.double() for t in C.kernel_inputs(shape, F64)]
    a = R.win2d_attention(qkv, table, B, H, W, heads, (wh, ww), (sh, sw))
    b = R.win2d_attention(qkv, table, B, H, W, heads, (wh, ww), (sh, sw), mask_value=float("-inf"))
    assert torch.equal(a, b)
    qkv, table = R.pinned_mask_case()
    S, _, tok = R.win2d_scores(qkv, table, 1, 1, 8, 1, (1, 8), (0, 4))
    P = S.softmax(-1)[0, 0, 0]                       # the map is one window
    _, reg = R.window_slots(1, 8, (1, 8), (0, 4))
    first, second = reg[0] == 0, reg[0] != 0
    assert first.sum() == 4 and second.sum() == 4
    assert float(P[first][:, second].sum(-1).min()) > 0.99
    inf = R.win2d_attention(qkv, table, 1, 1, 8, 1, (1, 8), (0, 4), mask_value=float("-inf"))
    assert rel(inf, R.win2d_attention(qkv, table, 1, 1, 8, 1, (1, 8), (0, 4))) > 0.5


# ====================================================================== the modules' trees
def test_module_trees_and_seeded_inits_are_the_forks(gold, swin):
    for tag, (kind, args, kwargs) in C.INIT.items():
        torch.manual_seed(C.INIT_SEED)
        sd = C.build(swin, kind, args, kwargs).state_dict()
        assert list(sd.keys()) == list(gold[f"init.{tag}.keys"])
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(gold[f"init.{tag}.shapes"])
        for (k, v), ref in zip(sd.items(), gold[f"init.{tag}.sums"]):
            # exact, but for the table: trunc_normal_ goes through erfinv, whose vectorised CPU code rounds differently from
            # one processor to the next (4e-9 seen on a sum of 0.27)
            assert abs(float(v.double().sum()) - float(ref)) <= (C.SUM_TOL * v.numel() if k.endswith("bias_table") else 0.0), k
        torch.manual_seed(C.INIT_SEED)
        sd = C.perturb(C.build(swin, kind, args, kwargs)).state_dict()
        pre = f"sd.{tag}."
        for k, v in sd.items():      # the perturbed seed-123 module IS the fixture's module, value for value
            ref = torch.from_numpy(gold[pre + k])
            assert torch.allclose(v, ref, rtol=0, atol=C.SUM_TOL) if k.endswith("bias_table") else torch.equal(v, ref), k
        m = C.build(swin, kind, args, kwargs)        # a fork checkpoint's entries load strictly
        m.load_state_dict({k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)}, strict=True)
    blk = C.build(swin, *C.INIT["block"])
    assert list(blk.state_dict().keys()) == [
        "norm1.weight", "norm1.bias", "attn.relative_position_bias_table", "attn.relative_position_index", "attn.qkv.weight",
        "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias",
        "mlp.3.weight", "mlp.3.bias"]
    assert blk.attn.relative_position_index.dtype == torch.int64
    assert torch.equal(blk.attn.relative_position_index, R.table_index((4, 8)))
    assert tuple(blk.attn.relative_position_bias_table.shape) == (7 * 15, 2)
    assert [n for n, _ in blk.named_children()] == ["norm1", "attn", "norm2", "mlp"]
    assert list(C.build(swin, *C.INIT["merge"]).state_dict().keys()) == ["reduce.weight", "norm.weight", "norm.bias"]
    assert list(C.build(swin, *C.INIT["comb"]).state_dict().keys()) == ["fc.weight", "fc.bias"]


def test_refusals(swin):
    ctors = {"attn": lambda **k: swin.WindowAttention2D(64, 2, (4, 8), **k),
             "block": lambda **k: swin.SwinBlock2D(64, 2, (4, 8), (0, 0), **k),
             "merge": lambda **k: swin.HeightOnlyPatchMerging(64, 128, **k),
             "comb": lambda **k: swin.Combining(64, 64, **k)}
    for tag, ctor in ctors.items():
        with pytest.raises(TypeError):
            ctor(compute_dtype=torch.float16)
        m = ctor().eval()
        x = torch.zeros(2, 32, 64)
        with pytest.raises(RuntimeError, match="runs on an MI355X only: move the module and its input to cuda"):
            m(x) if tag == "attn" else m(x, 4, 8)
        if tag != "attn":
            with pytest.raises(ValueError):          # N != H * W
                m(x, 4, 16)
    for ctor in (lambda *a: swin.WindowAttention2D(*a), lambda *a: swin.SwinBlock2D(*a, (0, 0))):
        with pytest.raises(ValueError):              # dim % num_heads
            ctor(100, 3, (4, 8))
        for dim, heads in ((32, 2), (96, 2), (512, 2)):      # head widths 16, 48, 256
            with pytest.raises(ValueError):
                ctor(dim, heads, (4, 8))
        for window in ((4, 9), (33, 1), (6, 6), (0, 8)):
            with pytest.raises(ValueError):
                ctor(64, 2, window)
    for shift in ((4, 0), (0, 8), (-1, 0), (2, 9)):
        with pytest.raises(ValueError):
            swin.SwinBlock2D(64, 2, (4, 8), shift)
    blk = swin.SwinBlock2D(64, 2, (4, 8), (2, 4)).eval()
    for H, W in ((6, 16), (8, 12)):                  # H % wh, W % ww
        with pytest.raises(ValueError):
            blk(torch.zeros(1, H * W, 64), H, W)
    with pytest.raises(NotImplementedError):
        swin.SwinBlock2D(64, 2, (4, 8), (0, 0), drop=0.1).train()(torch.zeros(1, 32, 64), 4, 8)
    with pytest.raises(NotImplementedError):
        swin.Combining(64, 64).train()(torch.zeros(1, 32, 64), 4, 8)         # the constructor's default drop=0.1
    with pytest.raises(NotImplementedError):
        swin.HeightOnlyPatchMerging(64, 128)(torch.zeros(1, 24, 64), 3, 8)
    with pytest.raises(NotImplementedError):
        swin.WindowAttention2D(64, 2, (4, 8))(torch.zeros(2, 32, 64), attn_mask=torch.zeros(2, 32, 32))


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
    assert "def window_attention_2d(qkv, table, B, H, W, heads, window, shift=(0, 0))" in var
    assert "def win2d_supported(head_dim, window, dtype)" in var
    assert os.path.exists(os.path.join(ROOT, "htr-vt_amd", "csrc", "swin.hip"))
