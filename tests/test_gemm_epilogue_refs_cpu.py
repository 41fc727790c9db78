"""What tests/gemm_epilogue_refs.py claims, checked without a GPU: the float64 forms against torch, the float32 emulation of
every rounding chain within 1.0 x its own error model on every random shape of tests/test_gemm_epilogue_gpu.py and on the
exhaustive bfloat16 sweep, and every mutant of the emulation (one rounding too many, tanh-GELU, a neighbour's bias, a side
tensor one row off in the last partial tile, GELU' at the unrounded value) ABOVE 1.0 on every one of those shapes -- the gate
of the GPU file tells them apart.  Run with -s for the worst ratio per (chain, form, output)."""
import collections

import pytest
import torch
import torch.nn.functional as F

import gemm_epilogue_refs as R

BF = torch.bfloat16
WORST = collections.defaultdict(float)


def plan(dtype):
    """(form, chain, float32 output) of every comparison on a case of operand type `dtype`"""
    if dtype == torch.float32:
        return [(f, "direct", True) for f in ("F1", "F2", "F3", "F4", "F5")]
    return [(f, c, False) for c in R.CHAINS for f in ("F1", "F2", "F3", "F4", "F5")] + \
           [(f, "direct", True) for f in ("F6", "F7r", "F7g", "F7d")]


def test_float64_forms_against_torch():
    x = torch.linspace(-9, 9, 3601, dtype=torch.float64).requires_grad_(True)
    y = F.gelu(x)
    assert (R.gelu64(x.detach()) - y.detach()).abs().max() < 1e-14
    y.sum().backward()
    assert (R.gelu_grad64(x.detach()) - x.grad).abs().max() < 1e-14
    case = R.random_case(37, 40, 64)
    a, b = case.A.double(), case.B.double()
    pre = F.linear(a, b, case.bias.double())
    assert torch.equal(R.reference(case, "F1").C, case.acc + case.bias.double())
    assert (R.reference(case, "F1").C - pre).abs().max() < 1e-13
    assert (R.reference(case, "F2").C - F.gelu(pre)).abs().max() < 1e-13 and (R.reference(case, "F2").preact - pre).abs().max() < 1e-13
    assert (R.reference(case, "F3").C - (pre + case.residual.double())).abs().max() < 1e-13
    xin = case.preact_in.double().requires_grad_(True)
    F.gelu(xin).backward(a @ b.t())
    assert (R.reference(case, "F4").C - xin.grad).abs().max() < 1e-13


def test_sweep_covers_every_small_bfloat16():
    v = R.sweep_values()
    assert v.numel() == 2 * (0x4101 + 4) and v.dtype == BF
    assert torch.isfinite(v.float()).all() and v.view(torch.int16).unique().numel() == v.numel()
    small = v.float().abs() <= 8
    assert int(small.sum()) == 2 * 0x4101                              # every pattern 0x0000 .. 0x4100 with either sign
    assert int((v.float() == 0).sum()) == 2 and int(((v.float() != 0) & (v.float().abs() < 2.0 ** -126)).sum()) == 2 * 127
    assert float(v.float().max()) == torch.finfo(BF).max


@pytest.mark.parametrize("M,N,K,dtype", R.random_shapes(), ids=lambda v: str(v).replace("torch.", ""))
def test_emulation_within_model_and_mutants_outside(M, N, K, dtype):
    base = R.random_case(M, N, K, dtype)
    for form, chain, f32_out in plan(dtype):
        case = R.as_f32_sides(base) if form in ("F7r", "F7d") else base
        ref, E = R.reference(case, form), R.error_model(case, form, chain, f32_out)
        tile_rows = 128 if chain == "direct" else 256
        em = R.emulate(case, form, chain, f32_out)
        for out, bound in E.items():
            ratio = R.worst_ratio(em[out], getattr(ref, out), bound)
            key = (chain, form if dtype == BF else form + "/f32", out)
            WORST[key] = max(WORST[key], ratio)
            assert ratio <= R.GATE, (form, chain, out, ratio)
        for mutant in R.mutants_of(form, chain, f32_out):
            mu = R.emulate(case, form, chain, f32_out, mutant=mutant, tile_rows=tile_rows)
            ratio = max(R.worst_ratio(mu[out], getattr(ref, out), bound) for out, bound in E.items())
            assert ratio > R.GATE, (form, chain, mutant, ratio)


@pytest.mark.parametrize("chain", list(R.CHAINS))
def test_emulation_on_the_bfloat16_sweep(chain):
    fast = R.CHAINS[chain][2]
    seen = 0
    for case in R.sweep_gelu_cases(264, 136, 64):
        x = case.acc
        assert torch.equal(x, case.B.double().t()[torch.arange(264) % 64] + 0.0)          # acc IS the swept value
        em = R.emulate(case, "F2", chain)
        assert torch.equal(em["preact"].double(), x)
        c = em["C"].double()
        assert torch.isfinite(c).all()
        assert torch.equal(c[x >= 6], x[x >= 6])
        ratio = R.worst_ratio(c, R.gelu64(x), R.sweep_bounds(x, "gelu", fast))
        WORST[(chain, "F2/sweep", "C")] = max(WORST[(chain, "F2/sweep", "C")], ratio)
        assert ratio <= R.GATE, ratio
        E = R.error_model(case, "F2", chain)
        assert R.worst_ratio(c, R.gelu64(x), E["C"]) <= R.GATE
        seen += 136 * 64
    assert seen >= R.sweep_values().numel()
    case = R.sweep_grad_case(264, 136, 64)
    assert torch.equal(case.acc, torch.ones(264, 136, dtype=torch.float64))
    c = R.emulate(case, "F4", chain)["C"].double()
    x = case.preact_in.double()
    assert torch.isfinite(c).all()
    ratio = R.worst_ratio(c, R.gelu_grad64(x), R.sweep_bounds(x, "grad", fast))
    WORST[(chain, "F4/sweep", "C")] = ratio
    assert ratio <= R.GATE, ratio
    assert R.worst_ratio(c, R.gelu_grad64(x), R.error_model(case, "F4", chain)["C"]) <= R.GATE


def test_integer_cases_are_exact_in_every_chain():
    case = R.integer_case(129, 40, 64)
    for chain in R.CHAINS:
        for form in ("F1", "F3"):
            assert torch.equal(R.emulate(case, form, chain)["C"].double(), R.reference(case, form).C)
    assert torch.equal(R.emulate(case, "F6", "direct")["C"].double(), R.reference(case, "F6").C)


def test_worst_ratios_are_the_recorded_ones():
    """(runs last) prints the worst ratio per (chain, form, output) over the tests of this session; the recorded ceilings of
    gemm_epilogue_refs.EMULATION_WORST must hold"""
    for key in sorted(WORST):
        print("EMULATION", *key, f"{WORST[key]:.3f}")
        assert WORST[key] <= R.GATE
        if key in R.EMULATION_WORST:
            assert WORST[key] <= R.EMULATION_WORST[key] + 0.02, (key, WORST[key])
