"""tests/conv_mixer_refs.py against tests/golden/conv_mixer.npz (arrays the fork's own ConvLocalMixer1D produced in
float64), the initial state_dict of htr-vt_amd/mixer.py against the fork's, and the new entry points' declarations.
No GPU: the package itself needs the built library to import, so mixer.py is loaded on a stub of its imports."""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import conv_mixer_cases as C
import conv_mixer_refs as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = ("htrvt_mixer_rows", "htrvt_mixer_fwd_workspace_floats", "htrvt_mixer_bwd_workspace_floats",
           "htrvt_mixer_reduce_rows", "htrvt_mixer_fwd_train", "htrvt_mixer_bn_silu", "htrvt_mixer_fwd_eval",
           "htrvt_mixer_bwd_reduce", "htrvt_mixer_bwd")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "conv_mixer.npz"))


def case_sd(gold, case, dtype=F64):
    use_bn = C.CASES[case][2]
    sd = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd.")}
    if not use_bn:
        sd = {k: v for k, v in sd.items() if not k.startswith("bn.")}
        sd["dwconv.bias"] = torch.from_numpy(gold["nobn.dwconv.bias"])
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


def rel(a, b):
    b = torch.as_tensor(b, dtype=F64)
    return float((a.double() - b).abs().max() / b.abs().max())


def load_mixer_module():
    """htr-vt_amd/mixer.py with its package imports stubbed: the module tree needs torch only"""
    pkg = types.ModuleType("_mixer_stub")
    pkg.__path__ = []
    subs = {"seq_ops": {"convert": None, "linear_wgrad": None}, "_lib": {"check": None, "lib": None},
            "ops": {"MNMAJOR": 1, "dt": None, "gemm": None, "ptr": None, "stream": None}}
    saved = {k: sys.modules.get(k) for k in ["_mixer_stub"] + ["_mixer_stub." + s for s in subs]}
    sys.modules["_mixer_stub"] = pkg
    for name, attrs in subs.items():
        m = types.ModuleType("_mixer_stub." + name)
        m.__dict__.update(attrs)
        sys.modules["_mixer_stub." + name] = m
        setattr(pkg, name, m)
    try:
        spec = importlib.util.spec_from_file_location("_mixer_stub.mixer", os.path.join(ROOT, "htr-vt_amd", "mixer.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@pytest.mark.parametrize("case", list(C.CASES))
def test_refs_reproduce_the_fork(gold, case):
    B, N, use_bn, _ = C.CASES[case]
    sd = case_sd(gold, case)
    x, dy = torch.from_numpy(gold[case + ".x"]).double(), torch.from_numpy(gold[case + ".dy"]).double()
    xs, dys = C.inputs(case)
    assert torch.equal(xs.double(), x) and torch.equal(dys.double(), dy)
    y_eval, _, _ = M.mixer_module(sd, x, training=False)
    assert rel(y_eval, gold[case + ".y_eval"]) < 1e-10
    y_train, rm, rv = M.mixer_module(sd, x, training=True)
    assert rel(y_train, gold[case + ".y_train"]) < 1e-10
    if use_bn:
        assert rel(rm, gold[case + ".running_mean"]) < 1e-10
        assert rel(rv, gold[case + ".running_var"]) < 1e-10
        assert int(gold[case + ".num_batches_tracked"]) == int(sd["bn.num_batches_tracked"]) + 1
    else:
        assert rm is None and rv is None
    dx, grads = M.mixer_module_grads(sd, x, dy, training=True)
    assert rel(dx, gold[case + ".dx"]) < 1e-10
    names = [k[len(case) + 6:] for k in gold.files if k.startswith(case + ".grad.")]
    assert sorted(names) == sorted(grads)
    for n in names:
        assert rel(grads[n], gold[f"{case}.grad.{n}"]) < 1e-10, n


def test_token_conv_is_the_forks_conv1d():
    g = torch.Generator().manual_seed(4)
    for B, N, D, k in ((2, 5, 8, 7), (3, 33, 24, 7), (1, 2, 8, 1), (2, 16, 16, 9)):
        x, w = torch.randn(B * N, D, generator=g, dtype=F64), torch.randn(D, k, generator=g, dtype=F64)
        assert rel(M.dwconv_tokens(x, w, B, N), M.fork_conv(x, w, B, N)) < 1e-12
        if B > 1:     # zero padding per image: another image's rows change nothing
            x2 = x.clone()
            x2[N:] += 1.0
            assert torch.equal(M.dwconv_tokens(x2, w, B, N)[:N], M.dwconv_tokens(x, w, B, N)[:N])


def test_core_backward_is_the_closed_form():
    """mixer_core_bwd (autograd) against the formulas the kernels use: dz = ds * silu'(z), the BatchNorm backward
    coefficients of kernel_refs.bn_bwd_coef, the flipped-tap convolution, the GLU backward"""
    import kernel_refs as R
    g = torch.Generator().manual_seed(6)
    B, N, D, k = 2, 5, 8, 7
    u, w, ds = (torch.randn(B * N, 2 * D, generator=g, dtype=F64), torch.randn(D, k, generator=g, dtype=F64),
                torch.randn(B * N, D, generator=g, dtype=F64))
    gamma, beta = torch.randn(D, generator=g, dtype=F64) + 1, torch.randn(D, generator=g, dtype=F64)
    rm, rv = torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)
    for training in (True, False):
        ref = M.mixer_core_bwd(ds, u, w, B, N, gamma, beta, rm, rv, training)
        c = M.glu_dwconv(u, w, B, N)
        if training:
            z, mean, rstd, _, _ = M.bn_train(c, gamma, beta, 1e-5, 0.1, rm, rv)
        else:
            mean, rstd = rm, 1.0 / torch.sqrt(rv + 1e-5)
            z = M.bn_eval(c, gamma, beta, 1e-5, rm, rv)
        scale = gamma * rstd
        shift = beta - mean * scale
        assert rel(M.affine(c, scale, shift), z) < 1e-12
        s1, s2 = M.bwd_sums(ds, c, scale, shift, mean, rstd)
        coef = R.bn_bwd_coef(s1, s2, float(B * N) if training else 0.0, gamma, mean, rstd)
        du, dw, _ = M.core_bwd(ds, c, u, w, B, N, scale, shift, coef)
        assert rel(dw, ref["dw"]) < 1e-10
        assert rel(du, ref["du"]) < 1e-10
        assert rel(s2, ref["dgamma"]) < 1e-10 and rel(s1, ref["dbeta"]) < 1e-10


def test_module_tree_and_seeded_init_are_the_forks(gold):
    mixer = load_mixer_module()
    for tag, use_bn in (("bn", True), ("nobn", False)):
        torch.manual_seed(C.INIT_SEED)
        sd = mixer.ConvLocalMixer1D(C.D, C.K, use_bn=use_bn).state_dict()
        assert list(sd.keys()) == list(gold[f"init.{tag}.keys"])
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(gold[f"init.{tag}.shapes"])
        np.testing.assert_array_equal(np.array([float(v.double().sum()) for v in sd.values()]), gold[f"init.{tag}.sums"])
    torch.manual_seed(C.INIT_SEED)
    m = C.perturb(mixer.ConvLocalMixer1D(C.D, C.K))
    sd = m.state_dict()
    assert len(sd) == 12 and tuple(sd["dwconv.weight"].shape) == (C.D, 1, C.K)
    for k, v in sd.items():          # the perturbed seed-123 module IS the fixture's module, value for value
        assert torch.equal(v, torch.from_numpy(gold["sd." + k])), k
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 5, C.D))
    with pytest.raises(ValueError):
        mixer.ConvLocalMixer1D(C.D, 6)


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    src = open(os.path.join(ROOT, "htr-vt_amd", "_lib.py")).read()
    seq = open(os.path.join(ROOT, "htr-vt_amd", "seq_ops.py")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", hdr), f"{name} is not declared in include/htrvt.h"
        assert f'"{name}"' in src, f"{name} has no ctypes prototype"
    assert "def conv_mixer_fwd(" in seq and "def conv_mixer_bwd(" in seq
    assert os.path.exists(os.path.join(ROOT, "htr-vt_amd", "csrc", "mixer.hip"))
