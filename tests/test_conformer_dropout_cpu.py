"""The convolutional forks' regularisers without a GPU: tests/conformer_dropout_refs.py (the float64 yardstick of
tests/test_conformer_dropout_gpu.py) with the masks the forks' own modules drew, against what those modules computed in
train mode (tests/golden/conformer_dropout.npz, float64) to 1e-10; the same refs with all-ones masks against
squeezeformer_refs; the host restatement of the masks; the new entry points' declarations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attn_dropout_refs as A
import conformer_dropout_refs as DR
import squeezeformer_cases as C
import squeezeformer_refs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NEW_SYMBOLS = ["htrvt_drop_add_ln_fwd", "htrvt_layernorm_bwd_drop"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "conformer_dropout.npz"))


def _close(name, got, ref, tol=1e-10):
    ref = torch.as_tensor(ref, dtype=F64)
    err = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
    assert err < tol, (name, err)


def _bits(gold, key, *shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(gold[key])[:n].reshape(shape).astype(np.float64))


def fixture_masks(gold, case):
    """(masks, rates) of a case in the form conformer_dropout_refs.run takes, from the fork's recorded draws"""
    kind, args, kwargs, B, N = DR.CASES[case]
    D = args[0]
    if kind == "ffn":
        return _bits(gold, case + ".E", B * N, D), kwargs["dropout"]
    if kind == "conv":
        return (_bits(gold, case + ".E", B * N, D), _bits(gold, case + ".S", B)), (kwargs["dropout"], kwargs["drop_path"])
    h, rates = args[1], DR.block_rates(case)
    if kind != "encoder":
        E, Sm, Am = _bits(gold, case + ".E", 4, B * N, D), _bits(gold, case + ".S", 4, B), _bits(gold, case + ".A", B, h, N, N)
        return dict(E=list(E), S=list(Sm), A=Am), rates
    n, Sm = N // 2, _bits(gold, case + ".S", 2, 4, B)
    E0, E1 = _bits(gold, case + ".E", 4, B * N, D), _bits(gold, case + ".E1", 4, B * n, D)
    A0, A1 = _bits(gold, case + ".A", B, h, N, N), _bits(gold, case + ".A1", B, h, n, n)
    return [dict(E=list(E0), S=list(Sm[0]), A=A0), dict(E=list(E1), S=list(Sm[1]), A=A1)], rates


def _case_sd(gold, case):
    from htrvt_amd import conformer
    sd = DR.case_module(conformer, case).state_dict()
    sums = gold[case + ".sdsum"]
    assert len(sums) == len(sd)
    for (k, v), s in zip(sd.items(), sums):
        assert abs(float(v.double().sum()) - float(s)) <= C.SUM_TOL * v.numel(), (case, k)
    return {k: v.double() for k, v in sd.items()}


@pytest.mark.parametrize("case", list(DR.CASES))
def test_refs_with_the_forks_masks_agree_with_the_fork(gold, case):
    """train-mode y (element by element for the two blocks, through the probe for every case), dx and every parameter
    gradient, 1e-10 of the tensor's largest magnitude; the fixture's masks really drop: every active mask has zeros"""
    kind, args = DR.CASES[case][:2]
    sd = _case_sd(gold, case)
    x, dy = [t.double() for t in DR.inputs(case)]
    masks, rates = fixture_masks(gold, case)
    y, dx, grads = DR.module_grads(kind, args, sd, x, dy, C.NORM_EPS, masks, rates)
    if case + ".y" in gold.files:
        _close(case + ".y", y, gold[case + ".y"])
    _close(case + ".y.gv", C.probe(y, True), gold[case + ".y.gv"])
    _close(case + ".dx.gv", C.probe(dx, True), gold[case + ".dx.gv"])
    pre = case + ".grad."
    assert set(grads) == {k[len(pre):-3] if k.endswith(".gv") else k[len(pre):] for k in gold.files if k.startswith(pre)}
    for n, g_ in grads.items():
        key = pre + n
        if key in gold.files:
            _close(key, g_.reshape(gold[key].shape), gold[key])
        else:
            _close(key + ".gv", C.probe(g_), gold[key + ".gv"])
    # and the masks matter: with none the output is far from the fixture's
    y0 = S.module_grads(kind, args, sd, x, dy, C.NORM_EPS)[0]
    assert float((C.probe(y0, True) - torch.from_numpy(gold[case + ".y.gv"])).abs().max()) > 1e-3


def test_the_fixture_draws_at_every_site(gold):
    """the blocks' recorded masks drop at every site, and every drop-path site keeps some sample and drops some"""
    for case in ("cblock", "sblock"):
        masks, rates = fixture_masks(gold, case)
        for i in range(4):
            share = 1.0 - float(masks["E"][i].mean())
            assert abs(share - rates["E"][i]) < 5 * (rates["E"][i] * (1 - rates["E"][i]) / masks["E"][i].numel()) ** 0.5
            assert 0 < float(masks["S"][i].sum()) < masks["S"][i].numel()
        assert abs(1.0 - float(masks["A"].mean()) - rates["A"]) < 5 * (0.09 / masks["A"].numel()) ** 0.5
        assert len({tuple(s.tolist()) for s in masks["S"]}) > 1          # four independent draws, not one


@pytest.mark.parametrize("case", list(DR.CASES))
def test_refs_with_all_ones_masks_are_the_rate_zero_refs(case):
    """keep everything, rates zero: conformer_dropout_refs.module_grads equals squeezeformer_refs.module_grads"""
    from htrvt_amd import conformer
    kind, args, _, B, N = DR.CASES[case]
    D = args[0]
    sd = {k: v.double() for k, v in DR.case_module(conformer, case).state_dict().items()}
    x, dy = [t.double() for t in DR.inputs(case)]
    if kind == "ffn":
        masks, rates = torch.ones(B * N, D, dtype=F64), 0.0
    elif kind == "conv":
        masks, rates = (torch.ones(B * N, D, dtype=F64), torch.ones(B, dtype=F64)), (0.0, 0.0)
    elif kind == "encoder":
        masks, rates = [DR.ones_masks(B, N, D, args[1]), DR.ones_masks(B, N // 2, D, args[1])], [DR.ZERO, DR.ZERO]
    else:
        masks, rates = DR.ones_masks(B, N, D, args[1]), DR.ZERO
    got = DR.module_grads(kind, args, sd, x, dy, C.NORM_EPS, masks, rates)
    ref = S.module_grads(kind, args, sd, x, dy, C.NORM_EPS)
    _close("y", got[0], ref[0], 1e-12)
    _close("dx", got[1], ref[1], 1e-12)
    assert set(got[2]) == set(ref[2])
    for n in ref[2]:
        _close(n, got[2][n], ref[2][n], 1e-12)


@pytest.mark.parametrize("p,p_path", [(0.1, 0.0), (0.0, 0.4), (0.5, 0.4)])
def test_host_masks(p, p_path):
    """the dropped share of the element mask is within 5 sigma of p, that of the sample mask (over many samples) within 5
    sigma of p_path; a rate of 0 keeps everything; the keys are (seed 0, row * D + col) and (seed 1, row // rows_per_sample)"""
    seeds, rows, D, rps = (0x1234567, 0x7654321), 4101, 264, 3
    e, s = DR.site_masks(seeds, rows, D, rps, p, p_path)
    assert e.shape == (rows, D) and s.shape == ((rows + rps - 1) // rps,)
    for m, q in ((e, p), (s, p_path)):
        if q == 0:
            assert m.all()
        else:
            assert abs(1.0 - m.mean() - q) <= 5 * (q * (1 - q) / m.size) ** 0.5
    if p > 0:
        assert bool(e[7, 5]) == bool(A.keep_elems(seeds[0], np.array([7 * D + 5]), p)[0])
    f = DR.site_factor(seeds, rows, D, rps, p, p_path)
    keep = torch.from_numpy(e & np.repeat(s, rps)[:rows, None])
    assert bool((f[~keep] == 0).all()) and torch.allclose(f[keep], torch.tensor(1.0 / (1 - p) / (1 - p_path), dtype=F64))


def test_kernel_restatement_is_autograd():
    """layernorm_bwd_drop's ds / dxb / dgamma / dbeta are the gradients of sum(LayerNorm(res + x * factor) * dy) at s, x, gamma
    and beta (plus dres at s)"""
    g = torch.Generator().manual_seed(3)
    rows, D = 9, 24
    x, res, dy, dres = [torch.randn(rows, D, generator=g, dtype=F64) for _ in range(4)]
    gamma, beta = torch.randn(D, generator=g, dtype=F64) + 1, torch.randn(D, generator=g, dtype=F64)
    f = DR.site_factor((11, 12), rows, D, 3, 0.5, 0.4)
    xl, rl, gl, bl = [t.clone().requires_grad_(True) for t in (x, res, gamma, beta)]
    s = DR.drop_add(xl, rl, f)
    y, mean, rstd = DR.drop_add_ln_fwd(s, gl, bl, 1e-6)
    ((y * dy).sum() + (s * dres).sum()).backward()
    ds, dxb, dgamma, dbeta = DR.layernorm_bwd_drop(dy, s.detach(), mean.detach(), rstd.detach(), gamma, dres, f)
    for n, a, b in zip(("ds", "dxb", "dgamma", "dbeta"), (ds, dxb, dgamma, dbeta), (rl.grad, xl.grad, gl.grad, bl.grad)):
        _close(n, a, b)


def test_abi_is_declared_and_exported():
    from htrvt_amd import _lib
    header = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.PROTOTYPES
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), sym), ctypes.c_void_p).value


def test_rates_reach_the_device_check_and_the_padded_attention_is_refused():
    """train mode serves every rate, on the device: the seeds are drawn there, so a host tensor is refused before any draw
    with an error that names the non-zero rates and the device (eval mode, and zero rates, reach the generic device check).
    What stays refused on the device is dropout on the attention probabilities where the attention pads its token count, and
    that refusal names the rate and N"""
    from htrvt_amd import conformer as M
    x = torch.zeros(2, 8, 64)
    mods = [(M.ConformerBlock(64, 2, 8, ff_dropout=0.1, attn_dropout=0.1, conv_dropout=0.1, drop_path=0.1),
             "ff_dropout = 0.1, attn_dropout = 0.1, conv_dropout = 0.1, drop_path = 0.1"),
            (M.SqueezeConformerBlock(64, 2, 8, drop_path=0.2), "ff_dropout = 0.1, conv_dropout = 0.1, drop_path = 0.2"),
            (M.SqueezeFormerEncoder(64, 2, 8, 2), "ff_dropout = 0.1, conv_dropout = 0.1"), (M.FeedForward(64, 128), "dropout = 0.1"),
            (M.ConvModule(64, drop_path=0.1), "dropout = 0.1, drop_path = 0.1")]
    for m, rates in mods:
        with pytest.raises(NotImplementedError, match=rates + " in train mode .*MI355X.* x is on cpu"):
            m.train()(x)
        with pytest.raises(RuntimeError, match="runs on an MI355X only"):
            m.eval()(x)
        assert m.last_drop_seeds is None
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):                  # every rate zero: nothing to draw
        M.ConformerBlock(64, 2, 8, ff_dropout=0.0).train()(x)
    enc = M.SqueezeFormerEncoder(64, 2, 8, 4)
    assert [b.drop_path_rate for b in enc._blocks()] == pytest.approx([0.0, 0.1 / 3, 0.2 / 3, 0.1])
    for dtype, N in ((torch.float32, 5), (torch.float32, 42), (torch.bfloat16, 20)):
        blk = M.ConformerBlock(64, 2, N, ff_dropout=0.0, attn_dropout=0.25, compute_dtype=dtype)
        with pytest.raises(NotImplementedError, match=rf"attn_dropout = 0\.25 .*N = {N} "):
            blk.train()(torch.zeros(1, N, 64))
        with pytest.raises(RuntimeError, match="MI355X"):
            blk.eval()(torch.zeros(1, N, 64))
    enc = M.SqueezeFormerEncoder(64, 2, 40, 2, attn_dropout=0.1, compute_dtype=torch.bfloat16)       # stage 2: 20 tokens
    with pytest.raises(NotImplementedError, match="N = 20 "):
        enc.train()(torch.zeros(1, 40, 64))
    with pytest.raises(RuntimeError, match="MI355X"):                                                  # float32 takes 20 as it is
        M.SqueezeFormerEncoder(64, 2, 40, 2, attn_dropout=0.1).train()(torch.zeros(1, 40, 64))
