"""tests/van_refs.py against torch's own depthwise convolution and against tests/golden/van.npz (arrays the fork's own
VANHeightReducer / HorizontalMixer produced in float64), the initial state_dict of htr-vt_amd/van.py against the fork's,
the constructor refusals, and the new entry points' declarations.
No GPU: the package itself needs the built library to import, so van.py is loaded on a stub of its imports."""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import van_cases as C
import van_refs as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = ("htrvt_van_dw_fwd", "htrvt_van_dw_bwd_input", "htrvt_van_dw_rows", "htrvt_van_dw_bwd_workspace_floats",
           "htrvt_van_dw_bwd_weight", "htrvt_van_moments_rows", "htrvt_van_moments", "htrvt_van_gate_fwd", "htrvt_van_gate_bwd",
           "htrvt_van_bn_res_gelu_fwd", "htrvt_van_bn_res_gelu_bwd", "htrvt_van_hpool_fwd", "htrvt_van_hpool_bwd")
SEQ_OPS = ("dwconv_fwd", "dwconv_bwd", "lka_fwd", "lka_bwd", "van_block_fwd", "van_block_bwd", "hmixer_fwd", "hmixer_bwd",
           "height_pool_fwd", "height_pool_bwd")
MODULES = {"red": ("van_reducer.", lambda sd, x, training: V.reducer(sd, x, training, C.DEPTH)),
           "mix": ("hmix.", V.hmixer)}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "van.npz"))


def module_sd(gold, prefix, dtype=F64):
    sd = {k[3 + len(prefix):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd." + prefix)}
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


def rel(a, b, scale=None):
    b = torch.as_tensor(b, dtype=F64)
    return float((a.double() - b).abs().max() / (b.abs().max() if scale is None else scale))


def grad_scale(gold, case, tag, name):
    """what a gradient's error is measured against: the largest reference magnitude of the tensor; for proj2.bias, whose
    gradient is a sum that cancels to rounding noise under the train-mode BatchNorm behind it, the fixture's magnitude of
    the sum's terms"""
    key = f"{case}.{tag}.gradscale.{name}"
    return float(gold[key]) if key in gold.files else None


def load_van_module():
    """htr-vt_amd/van.py with its package imports stubbed: the module tree needs torch only"""
    pkg = types.ModuleType("_van_stub")
    pkg.__path__ = []
    saved = {k: sys.modules.get(k) for k in ("_van_stub", "_van_stub.seq_ops")}
    seq = types.ModuleType("_van_stub.seq_ops")
    seq.convert = None
    sys.modules["_van_stub"], sys.modules["_van_stub.seq_ops"] = pkg, seq
    pkg.seq_ops = seq
    try:
        spec = importlib.util.spec_from_file_location("_van_stub.van", os.path.join(ROOT, "htr-vt_amd", "van.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


# ====================================================================== the operators
@pytest.mark.parametrize("shape", C.DW_SHAPES + [(2, 4, 16, 16, 7, 7, 3), (2, 5, 6, 8, 3, 9, 2), (1, 3, 4, 8, 1, 1, 1)])
def test_depthwise_refs_are_torchs_conv2d(shape):
    """forward, input gradient and weight gradient against F.conv2d(groups=C, dilation) and its autograd, float64"""
    B, H, W, Cc, kh, kw, dil = shape
    x, dy, w = [t.double() for t in C.dw_inputs(shape, F64)]
    xr, wr = x.permute(0, 3, 1, 2).clone().requires_grad_(True), V.conv2d_weight(w, kh, kw).clone().requires_grad_(True)
    y = F.conv2d(xr, wr, padding=((kh // 2) * dil, (kw // 2) * dil), dilation=dil, groups=Cc)
    (y * dy.permute(0, 3, 1, 2)).sum().backward()
    assert rel(V.dwconv(x, w, kh, kw, dil), y.detach().permute(0, 2, 3, 1)) < 1e-12
    assert rel(V.dwconv_bwd_input(dy, w, kh, kw, dil), xr.grad.permute(0, 2, 3, 1)) < 1e-12
    assert rel(V.dwconv_bwd_weight(x, dy, kh, kw, dil), wr.grad.reshape(Cc, kh * kw)) < 1e-12
    add = torch.randn(x.shape, dtype=F64, generator=torch.Generator().manual_seed(1))
    assert rel(V.dwconv_bwd_input(dy, w, kh, kw, dil, add=add), add + xr.grad.permute(0, 2, 3, 1)) < 1e-12
    if B > 1:      # zero padding per image: another image changes nothing
        x2 = x.clone()
        x2[1:] += 1.0
        assert torch.equal(V.dwconv(x2, w, kh, kw, dil)[:1], V.dwconv(x, w, kh, kw, dil)[:1])


def test_closed_form_backwards_are_autograd_of_the_forwards():
    (a, p, dg, res), scale, shift = C.ew_inputs((2, 3, 7, 24), F64)
    a, p, dg, res = [t.reshape(-1, 24) for t in (a, p, dg, res)]
    scale, shift = scale.double(), shift.double()
    ar, pr = a.clone().requires_grad_(True), p.clone().requires_grad_(True)
    z = V.affine(pr, scale, shift)
    z.retain_grad()
    (ar * z * dg).sum().backward()
    da, dz = V.gate_bwd(dg, a, p, scale, shift)
    assert rel(da, ar.grad) < 1e-12 and rel(dz, z.grad) < 1e-12
    assert rel(V.gate_fwd(a, p, scale, shift), (ar * z).detach()) < 1e-12
    for r in (res, None):
        pr = p.clone().requires_grad_(True)
        z = V.affine(pr, scale, shift)
        t = z if r is None else r + z
        t.retain_grad()
        y = F.gelu(t)
        (y * dg).sum().backward()
        assert rel(V.bn_res_gelu_fwd(p, scale, shift, r), y.detach()) < 1e-12
        assert rel(V.bn_res_gelu_bwd(dg, p, scale, shift, r), t.grad) < 1e-12
    x = C.ew_inputs((2, 3, 7, 24), F64)[0][0]
    xr = x.clone().requires_grad_(True)
    y = F.adaptive_avg_pool2d(xr.permute(0, 3, 1, 2), (1, None))          # (B, C, 1, W), as the fork pools
    d = torch.randn(2, 7, 24, dtype=F64, generator=torch.Generator().manual_seed(2))
    (y[:, :, 0].permute(0, 2, 1) * d).sum().backward()
    assert rel(V.hpool_fwd(x), y.detach()[:, :, 0].permute(0, 2, 1)) < 1e-12
    assert rel(V.hpool_bwd(d, 3), xr.grad) < 1e-12
    m = V.moments(a)
    assert m.shape == (1, 2, 24) and rel(m[0, 0], a.sum(0)) < 1e-12 and rel(m[0, 1], (a * a).sum(0)) < 1e-12


# ====================================================================== the modules
@pytest.mark.parametrize("tag", list(MODULES))
@pytest.mark.parametrize("case", list(C.CASES))
def test_refs_reproduce_the_fork(gold, case, tag):
    prefix, fn = MODULES[tag]
    sd = module_sd(gold, prefix)
    ins = C.inputs(case)
    for t, n in zip(ins, ("x", "dy", "xm", "dym")):
        assert torch.equal(t, torch.from_numpy(gold[f"{case}.{n}"]))
    x, dy = [t.double() for t in (ins[:2] if tag == "red" else ins[2:])]
    pre = f"{case}.{tag}."
    y_eval, buffers = fn(sd, x, False)
    assert rel(y_eval, gold[pre + "y_eval"]) < 1e-10 and not buffers
    y_train, buffers = fn(sd, x, True)
    assert rel(y_train, gold[pre + "y_train"]) < 1e-10
    names = [k[len(pre) + 4:] for k in gold.files if k.startswith(pre + "buf.")]
    assert sorted(names) == sorted(buffers) and len(names) == (12 if tag == "red" else 3)
    for n in names:
        if n.endswith("num_batches_tracked"):
            assert int(buffers[n]) == int(gold[pre + "buf." + n]) == int(sd[n]) + 1
        else:
            assert rel(buffers[n], gold[pre + "buf." + n]) < 1e-10, n
    dx, grads = V.module_grads(lambda s, t: fn(s, t, True), sd, x, dy)
    assert rel(dx, gold[pre + "dx"]) < 1e-10
    names = [k[len(pre) + 5:] for k in gold.files if k.startswith(pre + "grad.")]
    assert sorted(names) == sorted(grads)
    for n in names:
        assert rel(grads[n], gold[pre + "grad." + n], grad_scale(gold, case, tag, n)) < 1e-10, n


def test_module_trees_and_seeded_inits_are_the_forks(gold):
    van = load_van_module()
    build = {"reducer": (lambda: van.VANHeightReducer(C.D, depth=C.DEPTH), "van_reducer."),
             "hmix": (lambda: van.HorizontalMixer(C.D, k=C.K), "hmix.")}
    for tag, (ctor, prefix) in build.items():
        torch.manual_seed(C.INIT_SEED)
        sd = ctor().state_dict()
        assert list(sd.keys()) == list(gold[f"init.{tag}.keys"])
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(gold[f"init.{tag}.shapes"])
        np.testing.assert_array_equal(np.array([float(v.double().sum()) for v in sd.values()]), gold[f"init.{tag}.sums"])
        torch.manual_seed(C.INIT_SEED)
        sd = C.perturb(ctor()).state_dict()
        for k, v in sd.items():      # the perturbed seed-123 module IS the fixture's module, value for value
            assert torch.equal(v, torch.from_numpy(gold["sd." + prefix + k])), k
        m = ctor()                   # a fork checkpoint's entries load strictly
        m.load_state_dict({k[3 + len(prefix):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd." + prefix)},
                          strict=True)
    assert len(build["reducer"][0]().state_dict()) == 2 * 17 and len(build["hmix"][0]().state_dict()) == 7
    lka, blk = van.LargeKernelAttention(8), van.VANBlock(8, drop_path=0.1)
    assert tuple(lka.dwd.weight.shape) == (8, 1, 7, 7) and lka.dwd.dilation == (3, 3) and lka.dwd.padding == (9, 9)
    assert [n for n, _ in blk.named_children()] == ["proj1", "act", "lka", "proj2", "norm", "drop_path"]


def test_refusals():
    van = load_van_module()
    for ctor in (van.LargeKernelAttention, van.VANBlock, van.VANHeightReducer, van.HorizontalMixer):
        with pytest.raises(ValueError):
            ctor(12)
        with pytest.raises(TypeError):
            ctor(8, compute_dtype=torch.float16)
        with pytest.raises(RuntimeError, match="runs on an MI355X only: move the module and its input to cuda"):
            ctor(8)(torch.zeros(2, 8, 1, 5))
    with pytest.raises(NotImplementedError):
        van.VANHeightReducer(8, pool="max")
    with pytest.raises(ValueError, match="Unsupported pool type: median"):
        van.VANHeightReducer(8, pool="median")
    for k in (0, 4, 11):
        with pytest.raises(ValueError):
            van.HorizontalMixer(8, k=k)
    blk = van.VANBlock(8, drop_path=0.1)
    with pytest.raises(NotImplementedError):
        blk.train().forward_nhwc(torch.zeros(1, 1, 2, 8))


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
    assert "def depthwise_conv2d(x_nhwc, weight, dilation=1)" in var
    assert os.path.exists(os.path.join(ROOT, "htr-vt_amd", "csrc", "van.hip"))
