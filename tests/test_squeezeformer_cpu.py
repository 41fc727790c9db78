"""The convolutional forks' blocks without a GPU: tests/squeezeformer_refs.py (the float64 yardstick of the GPU tests) against
tests/golden/squeezeformer.npz (the fork's own modules in float64) to 1e-10, the new C ABI's declarations, and the module
trees, seeded initial values and refusals of htrvt_amd.conformer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import squeezeformer_cases as C
import squeezeformer_refs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NEW_SYMBOLS = ["htrvt_gnmixer_rows", "htrvt_gnmixer_parts", "htrvt_gnmixer_fwd", "htrvt_gn_finalize", "htrvt_gnmixer_act",
               "htrvt_gnmixer_bwd_reduce", "htrvt_gn_bwd_finalize", "htrvt_gnmixer_bwd", "htrvt_se_mean", "htrvt_se_mlp_fwd",
               "htrvt_se_scale_fwd", "htrvt_se_scale_bwd_reduce", "htrvt_se_mlp_bwd", "htrvt_se_wgrad", "htrvt_se_scale_bwd",
               "htrvt_seq_down2_fwd", "htrvt_seq_down2_bwd", "htrvt_seq_up_add_fwd", "htrvt_seq_up_add_bwd", "htrvt_silu_fwd",
               "htrvt_silu_bwd"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "squeezeformer.npz"))


def _close(name, got, ref, tol=1e-10):
    ref = torch.as_tensor(ref, dtype=F64)
    err = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
    assert err < tol, (name, err)


def _against(gold, key, t, activation=False):
    """t against the fixture's entry: element by element, or through the probe where the fixture keeps only that"""
    if key in gold.files:
        _close(key, t.reshape(gold[key].shape), gold[key])
    else:
        _close(key + ".gv", C.probe(t, activation), gold[key + ".gv"])


def _case_sd(gold, case):
    """the case's state_dict in float64, checked against the fixture's per-key sums"""
    from htrvt_amd import conformer
    sd = C.case_module(conformer, case).state_dict()
    sums = gold[case + ".sdsum"]
    assert len(sums) == len(sd)
    for (k, v), s in zip(sd.items(), sums):
        assert abs(float(v.double().sum()) - float(s)) <= C.SUM_TOL * v.numel(), (case, k)
    return {k: v.double() for k, v in sd.items()}


@pytest.mark.parametrize("case", list(C.CASES))
def test_refs_agree_with_the_fork(gold, case):
    """outputs, dx and every parameter gradient of every module, 1e-10 of the tensor's largest magnitude"""
    kind, args = C.CASES[case][:2]
    sd = _case_sd(gold, case)
    x, dy = [t.double() for t in C.inputs(case)]
    y, dx, grads = S.module_grads(kind, args, sd, x, dy, C.NORM_EPS, C.UP_TARGET.get(case))
    _against(gold, case + ".y", y, True)
    _against(gold, case + ".dx", dx, True)
    pre = case + ".grad."
    assert set(grads) == {k[len(pre):-3] if k.endswith(".gv") else k[len(pre):] for k in gold.files if k.startswith(pre)}
    for n, g_ in grads.items():
        _against(gold, f"{case}.grad.{n}", g_)


def test_per_image_statistics_and_the_surviving_bias():
    """gn_mixer is F.group_norm(1 group) over the fork's [B, C, N] layout behind a biased depthwise Conv1d; dropping the bias or
    taking batch-wide statistics is far outside 1e-10"""
    B, N, Cc, k = 3, 7, 8, 5
    u, _, w, bias, gamma, beta = [t.double() for t in C.mixer_inputs(B, N, Cc, k, torch.float32)]
    g = F.glu(u.view(B, N, 2 * Cc).transpose(1, 2), dim=1)
    c = F.conv1d(g, w[:, None], bias, padding=k // 2, groups=Cc)
    ref = F.silu(F.group_norm(c, 1, gamma, beta, 1e-5)).transpose(1, 2).reshape(B * N, Cc)
    _close("gn_mixer", S.gn_mixer(u, w, bias, gamma, beta, B, N), ref)
    assert float((S.gn_mixer(u, w, torch.zeros_like(bias), gamma, beta, B, N) - ref).abs().max()) > 1e-3
    assert float((S.gn_mixer(u, w, bias, gamma, beta, 1, B * N) - ref).abs().max()) > 1e-3


def test_staged_backward_is_autograd():
    """the launches' closed forms (sums, means, dc, du, dw, db, d gamma, d beta) against autograd through gn_mixer"""
    B, N, Cc, k = 3, 7, 8, 5
    u, ds, w, bias, gamma, beta = [t.double() for t in C.mixer_inputs(B, N, Cc, k, torch.float32)]
    c = S.gn_conv(u, w, bias, B, N)
    mean, rstd = S.gn_stats(c, B, N, 1e-5)
    s1, s2, p1, p2 = S.gn_bwd_sums(ds, c, mean, rstd, gamma, beta, B, N)
    du, dw, db = S.gn_core_bwd(ds, c, u, w, mean, rstd, gamma, beta, p1 / (Cc * N), p2 / (Cc * N), B, N)
    ref = S.grads_of(lambda *a: S.gn_mixer(*a, B, N), ds, u, w, bias, gamma, beta)
    for n, a, b in zip(("du", "dw", "dbias", "dgamma", "dbeta"), (du, dw, db, s2, s1), ref):
        _close(n, a, b)


def test_staged_squeeze_excite_backward_is_autograd():
    B, N, D = 3, 5, 24
    x, dy, w1, b1, w2, b2 = [t.double() for t in C.se_inputs(B, N, D, torch.float32)]
    mean = S.se_mean(x, B, N)
    pre, act, g = S.se_mlp(mean, w1, b1, w2, b2)
    dh2, dh1, dmean = S.se_mlp_bwd(S.se_dg(dy, x, B, N), g, pre, w1, w2)
    got = (S.se_dx(dy, g, dmean, N),) + S.se_wgrad(dh1, mean) + S.se_wgrad(dh2, act)
    ref = S.grads_of(lambda *a: S.se(*a, B, N), dy, x, w1, b1, w2, b2)
    for n, a, b in zip(("dx", "dw1", "db1", "dw2", "db2"), got, ref):
        _close(n, a, b)


def test_up_sampling_index_is_torch_nearest():
    """(i * n) // N0 equals F.interpolate(mode='nearest') for every N0 in 2 ... 1099 with n = N0 // 2, and for the fixture's
    other lengths"""
    pairs = [(N0 // 2, N0) for N0 in range(2, 1100)] + [(2, 5), (16, 33), (1, 7), (5, 5)]
    for n, N0 in pairs:
        src = F.interpolate(torch.arange(n, dtype=F64).view(1, 1, n), size=N0, mode="nearest").view(-1).long()
        assert torch.equal(S.up_index(n, N0), src), (n, N0)


def test_down_sampling_is_avg_pool():
    for N in (2, 5, 33):
        x = torch.randn(3 * N, 8, dtype=F64)
        ref = F.avg_pool1d(x.view(3, N, 8).transpose(1, 2), 2, 2).transpose(1, 2).reshape(-1, 8)
        _close("down2", S.down2(x, 3, N), ref)
    assert S.down2(x[:3], 3, 1) is x[:3] or torch.equal(S.down2(x[:3], 3, 1), x[:3])


def test_abi_is_declared_and_exported():
    from htrvt_amd import _lib
    header = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.PROTOTYPES
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), sym), ctypes.c_void_p).value       # the built library exports it


@pytest.mark.parametrize("tag", list(C.INIT))
def test_state_dict_matches_the_fork_init(gold, tag):
    """keys in order, shapes, and the seeded initial values (per-key sums)"""
    from htrvt_amd import conformer
    kind, args, kwargs = C.INIT[tag]
    torch.manual_seed(C.INIT_SEED)
    sd = C.build(conformer, kind, args, kwargs).state_dict()
    assert list(sd.keys()) == list(gold[f"init.{tag}.keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(gold[f"init.{tag}.shapes"])
    for (k, v), s in zip(sd.items(), gold[f"init.{tag}.sums"]):
        assert abs(float(v.double().sum()) - float(s)) <= C.SUM_TOL * v.numel(), k
    if kind == "conv":
        assert tuple(sd["pointwise_conv1.weight"].shape) == (32, 32, 1)


def test_refusals():
    from htrvt_amd import conformer as M
    with pytest.raises(ValueError, match="multiples of 8"):
        M.ConvModule(24)                      # GLU output 12
    with pytest.raises(ValueError, match="odd"):
        M.ConvModule(30, expansion=0.5)       # hidden_channels 15: the fork's path without GLU
    for k in (0, 4, 17):
        with pytest.raises(ValueError, match="kernel_size"):
            M.ConvModule(32, kernel_size=k)
    with pytest.raises(TypeError):
        M.ConvModule(32, compute_dtype=torch.float16)
    x = torch.zeros(1, 4, 64)
    for kw in (dict(ff_dropout=0.1), dict(ff_dropout=0.0, attn_dropout=0.1), dict(ff_dropout=0.0, drop_path=0.1)):
        for ctor in (M.ConformerBlock, M.SqueezeConformerBlock):
            blk = ctor(64, 2, 4, **kw)
            with pytest.raises(NotImplementedError, match="train mode"):
                blk.train()(x)
            with pytest.raises(RuntimeError, match="MI355X"):       # eval mode gets as far as the device check
                blk.eval()(x)
    enc = M.SqueezeFormerEncoder(64, 2, 4, 2)                        # the fork's defaults: ff_dropout 0.1, drop_path_total 0.1
    with pytest.raises(NotImplementedError, match="train mode"):
        enc.train()(x)
    with pytest.raises(NotImplementedError, match="train mode"):
        M.FeedForward(32, 64).train()(torch.zeros(1, 4, 32))
    with pytest.raises(NotImplementedError, match="drop_path"):
        M.ConvModule(32, drop_path=0.1).train()(torch.zeros(1, 4, 32))
    with pytest.raises(RuntimeError, match="MI355X"):
        M.ConvModule(32).train()(torch.zeros(1, 4, 32))
    with pytest.raises(ValueError, match="head width"):
        M.ConformerBlock(64, 4, 4)
