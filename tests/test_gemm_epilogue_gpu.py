"""The Linear epilogues of htrvt_gemm in every kernel family, element by element against float64 (tests/gemm_epilogue_refs.py;
tests/test_gemm_epilogue_refs_cpu.py proves the references, the error model and that the gate tells the mutants apart).

Families (csrc/gemm.hip launch_main, gemm8p.hip, gemm_dma.hip): the 8-phase kernels with 256 / 192 columns, their persistent
form, the LDS-DMA kernels with 192 / 128 (two and three stages) / 64 / 256 columns, the routes the library takes on its own
for few-row Linear launches and where the 8-phase family declines, and the register-staged 128-row kernel in bfloat16 and
float32.  route() restates the library's choice for a plain Linear launch; EVERY launch is attributed through
htrvt_last_kernel() to the symbol route() names -- where a family declines a form (float32 C with side tensors, GELU' on the
persistent kernel, ...) that is the kernel that took it, with ITS rounding chain.

Every launch: ldc = N + 8 shared by C, preact and residual; C and preact cut out of a larger allocation and pre-filled with
NaN; the pad columns keep the fill, the guard bands their pattern, no NaN is left inside, a second launch gives the same
bits; every element within GATE = 1.0 x the error model of the chain that served it.  The exhaustive bfloat16 sweep holds
the two packed polynomials (and libm's erff on the other chain) to their stated errors on the device, the integer cases are
exact.  Each comparison prints `RATIO <family> <form> <output> <worst>` (pytest -s).

Worst |got - float64| / bound per (chain, form, output), MI355X over every case of this file | host emulation (CPU test):
(rows: the family the case list names; a form a family declines is counted with the kernel that took it.  F2 pre / F7g pre: the
saved pre-activation.  swp: the exhaustive bfloat16 sweep against its own gate.  Float32 outputs sit far below 1 because the
accumulation term 2 K 2^-24 is a worst-case bound.)
                      F1      F2  F2 pre      F3      F4      F5      F6     F7r     F7g F7g pre     F7d  F2 swp  F4 swp
    8p256           0.99    0.95    0.99    0.99    0.98    0.95    0.01    0.02    0.13    0.01    0.19    0.97    0.99
    8p192           0.99    0.95    0.99    0.99    0.99    0.95    0.02    0.02    0.14    0.02    0.18    0.97    0.99
    dma192          0.99    0.95    0.99    0.98    0.95    0.95    0.01    0.02    0.14    0.01    0.19    0.97    0.99
    dma192_lw       0.99    0.95    0.99    0.98    0.95    0.95    0.01    0.02    0.14    0.01    0.19    0.97    0.99
    dma128_s2       0.99    0.95    0.99    0.97    0.96    0.95    0.01    0.02    0.13    0.01    0.17    0.97    0.99
    dma128_s3       0.99    0.95    0.99    0.97    0.96    0.95    0.01    0.02    0.13    0.01    0.17    0.97    0.99
    dma64           0.98    0.93    0.98    0.94    0.91    0.93    0.01    0.02    0.11    0.01    0.13    0.97    0.99
    dma256          0.99    0.99    0.99    0.99    0.98    0.99    0.01    0.02    0.10    0.01    0.15    0.97    0.99
    auto_small_m    0.99    0.95    0.99    0.99    0.96    0.95    0.01    0.02    0.16    0.01    0.21    0.97    0.99
    auto_decline    0.99    0.95    0.99    0.98    0.95    0.95    0.01    0.02    0.14    0.01    0.20    0.97    0.99
    reg_auto        0.99    0.99    0.99    0.98    0.98    0.99    0.01    0.02    0.14    0.01    0.14    0.97    0.99
    reg_bf16        0.99    0.98    0.99    0.99    0.99    0.98    0.01    0.02    0.13    0.01    0.17    0.97    0.99
    reg_f32         0.03    0.13    0.03    0.03    0.17    0.13                                            0.20    0.21
    pp256           0.97    0.94    0.97    0.98    0.97    0.94                                            0.97    0.99
    pp192           0.97    0.94    0.97    0.98    0.97    0.94                                            0.97    0.99
    pp_auto_1032    0.97    0.94    0.97    0.98    0.97    0.94
    pp_auto_780     0.95    0.95    0.95    0.97    0.95    0.95
  host emulation (gemm_epilogue_refs.EMULATION_WORST), per chain:
    acc             0.99    0.95    0.99    0.99    0.99    0.95                                            0.97    0.99
    staged          0.99    0.95    0.99    0.99    0.96    0.95                                            0.97    0.99
    direct          0.99    0.99    0.99    0.99    0.99    0.99    0.02    0.02    0.13    0.02    0.19    0.98    0.99
    direct, float32 operands
                    0.03    0.12    0.03    0.03    0.19    0.12
-- every family stays where the emulation of ITS chain (route() names it per launch) is: no family rounds at a point the
table of gemm_epilogue_refs lacks.  The sweep ran on the kernels with the tail fix of gelu_erf_fast2 (csrc/gemm_common.h);
before it F2 failed at x = -100, -9984 and the largest finite bfloat16 on every family that uses the polynomial.
"""
import functools

import pytest
import torch

import gemm_epilogue_refs as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
E_RES, E_GELU, E_GELUGRAD, E_F32 = 1, 2, 4, 128          # csrc/gemm_common.h
PAD = 8                                                  # ldc = N + PAD


def _ops():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import ops
    return ops


def _last_kernel():
    from htrvt_amd._lib import lib
    return lib.htrvt_last_kernel().decode()


@functools.lru_cache(maxsize=None)
def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7


def _ceil(a, b):
    return (a + b - 1) // b


def route(tile, dtype, M, N, K, ldc, form, b_mn=False):
    """(kernel symbol, rounding chain) of a plain Linear launch: the choice of csrc/gemm.hip launch_main restated --
    gemm8p.hip gemm8p_serves / gemm8p_pick_bn / the persistent test of gemm8p_try_launch, gemm_dma.hip pick_bn /
    use_loader_waves, the staged-or-direct test at the end of gemm_dma_body, gemm.hip pick_tile"""
    f32 = form in R.F32_OUT
    act, _, _, with_res, _ = R.FORM_SPEC[form]
    if dtype == F32 or tile == 1 or M <= 128:
        bn = 64 if N <= 64 else (192 if N % 192 == 0 and N % 128 != 0 else 128)
        return f"gemm_kernel<{'float' if dtype == F32 else 'bf16_t'}, 128, {bn}, 0, {int(b_mn)}, 0>", "direct"
    tm = _ceil(M, 256)
    small = tile == 0 and not b_mn and N <= 1024 and N % 128 == 0 and tm * _ceil(N, 192) <= 128
    if tile in (0, 9, 10, 11, 13, 14, 15) and not small and not b_mn:
        if tile in (10, 14):
            bn = 256
        elif tile in (11, 15):
            bn = 192
        else:
            cost = lambda w, per: _ceil(tm * _ceil(N, w), 256) * w * per      # noqa: E731
            bn = 192 if cost(192, 1.12) < cost(256, 1.0) else 256
        if N % (8 if bn == 256 else 12) == 0 and ldc % 4 == 0 and not (f32 and (act != 0 or with_res)):
            epi = E_F32 if f32 else {0: 0, 1: E_GELU, 2: E_GELUGRAD}[act] | (E_RES if with_res else 0)
            cfg = "Cfg<256, 2, 4>" if bn == 256 else "Cfg<192, 4, 2>"
            res_ok = epi == E_RES and bn == 192 and K >= 256
            want = tile in (13, 14, 15) or (tile == 0 and (epi == 0 or res_ok))
            if want and (epi in (0, E_GELU) or res_ok) and K % 128 == 0 and K >= 256 and tm * _ceil(N, bn) >= _ncu():
                return f"gemm8pp_kernel<{cfg}, {epi}>", "acc"
            return f"gemm8p_kernel<{cfg}, 0, {epi}>", "acc"
    if tile == 6 and N % 256 == 0:
        bn = 256
    elif N <= 64:
        bn = 64
    elif N <= 128 or tile in (7, 8) or small:
        bn = 128
    else:
        bn = 192 if _ceil(N, 192) * 192 <= _ceil(N, 128) * 128 else 128
    spec = 0 if bn == 256 or tile == 3 else (1 if tile == 4 else int(K >= 2048))
    nstage = 3 if bn == 128 and (tile == 8 or small) else 2
    staged = bn <= 192 and not f32 and (ldc | N) % 8 == 0
    return f"gemm_dma_kernel<256, {bn}, 0, {int(b_mn)}, 0, {spec}, {nstage}>", "staged" if staged else "direct"


def _padded(t, ld, fill):
    """[rows, cols] host tensor -> device [rows, ld] with `fill` in the pad columns"""
    rows, cols = t.shape
    d = torch.full((rows, ld), fill, dtype=t.dtype)
    d[:, :cols] = t
    return d.cuda()


def launch(case, form, tile, b_mn=False, ldb_pad=0, a_off=0):
    """one htrvt_gemm of `form` on `case` -> (C, preact or None, kernel symbol); C / preact are [M, N + PAD] guarded tensors"""
    ops = _ops()
    M, N, K, dtype = case.M, case.N, case.K, case.dtype
    act, with_bias, saves, with_res, with_pre = R.FORM_SPEC[form]
    f32 = form in R.F32_OUT
    cdt = F32 if (f32 or dtype == F32) else BF
    ldc = N + PAD
    lda = K + (2 * a_off if a_off else 0)
    a = torch.full((M, lda), 3.0, dtype=dtype)
    a[:, a_off:a_off + K] = case.A
    a = a.cuda()
    if b_mn:
        b, ldb = case.B.t().contiguous().cuda(), N
    else:
        b, ldb = _padded(case.B, K + ldb_pad, 3.0), K + ldb_pad
    c = R.guarded((M, ldc), cdt)
    kw = {}
    if with_bias and case.bias is not None:
        kw["bias"] = case.bias.cuda()
    if saves:
        kw["preact"] = R.guarded((M, ldc), cdt)
    if with_res:
        kw["residual"] = _padded(case.residual.to(cdt), ldc, 5.0)
    if with_pre:
        kw["preact"] = _padded(case.preact_in.to(cdt), ldc, 5.0)
    ops.gemm(a, b, c, dtype=dtype, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, alpha=case.alpha, act=act, c_f32=f32, tile=tile,
             a_off=a_off, b_layout=ops.MNMAJOR if b_mn else ops.KMAJOR, **kw)
    return c, (kw["preact"] if saves else None), _last_kernel()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def run(family, case, form, tile, **kw):
    """two launches; attribution, pad columns, guards, NaN, same bits -> (outputs as float64 [M, N] on the host, chain)"""
    M, N = case.M, case.N
    want, chain = route(tile, case.dtype, M, N, case.K, N + PAD, form, b_mn=kw.get("b_mn", False))
    c1, p1, k1 = launch(case, form, tile, **kw)
    c2, p2, k2 = launch(case, form, tile, **kw)
    assert want in k1 and k1 == k2, (family, form, want, k1, k2)
    R.assert_guards_intact()
    outs = {}
    for name, t1, t2 in (("C", c1, c2), ("preact", p1, p2)):
        if t1 is None:
            continue
        assert torch.isnan(t1[:, N:]).all(), (family, form, name, "a store into the pad columns")
        assert not torch.isnan(t1[:, :N]).any(), (family, form, name, "an element was not written")
        assert torch.equal(_bits(t1), _bits(t2)), (family, form, name, "two launches differ")
        outs[name] = t1[:, :N].double().cpu()
    return outs, chain, c1, p1


def check(family, case, form, tile, **kw):
    cs = R.as_f32_sides(case) if form in ("F7r", "F7d") else case
    outs, chain, _, _ = run(family, cs, form, tile, **kw)
    f32_out = form in R.F32_OUT or case.dtype == F32
    ref, E = R.reference(cs, form), R.error_model(cs, form, chain, f32_out)
    for name, bound in E.items():
        ratio = R.worst_ratio(outs[name], getattr(ref, name), bound)
        print(f"RATIO {family} {form} {name} {ratio:.3f} [{chain}{'/f32' if f32_out else ''}]")
        assert ratio <= R.GATE, (family, form, name, chain, ratio)


def forms_of(dtype):
    return ("F1", "F2", "F3", "F4", "F5") if dtype == F32 else R.FORMS


# ---- random cases ------------------------------------------------------------------------------------------------------
RANDOM = [(name, M, N, K) for name, fam in R.FAMILIES.items() for M in fam["Ms"] for N in fam["Ns"] for K in fam["Ks"]]


@pytest.mark.parametrize("family,M,N,K", RANDOM)
def test_random(family, M, N, K):
    fam = R.FAMILIES[family]
    case = R.random_case(M, N, K, fam["dtype"])
    for form in forms_of(fam["dtype"]):
        check(family, case, form, fam["tile"])


def _persistent_rows(bn_tiles=5):
    """M = 256 t + 1 with (t + 1) x 5 tiles >= CUs + 4: more tiles than workgroups, a one-row last row tile"""
    return 256 * (_ceil(_ncu() + 4, bn_tiles) - 1) + 1


@pytest.mark.parametrize("family,K", [("pp256", 256), ("pp256", 384), ("pp192", 256), ("pp192", 384), ("pp_auto_1032", 256),
                                      ("pp_auto_780", 384)])
def test_random_persistent(family, K):
    fam = R.PERSISTENT[family]
    M, N = _persistent_rows(), fam["N"]
    case = R.random_case(M, N, K)
    served = [route(fam["tile"], BF, M, N, K, N + PAD, form)[0] for form in ("F1", "F2", "F3")]
    if family in ("pp256", "pp192"):          # the family under test did take what it serves
        assert "gemm8pp_kernel" in served[0] and "gemm8pp_kernel" in served[1], served
        assert ("gemm8pp_kernel" in served[2]) == (family == "pp192"), served
    for form in ("F1", "F2", "F3", "F4", "F5"):       # (float32 C never reaches the persistent kernel: covered at the small shapes)
        check(family, case, form, fam["tile"])


# ---- the exhaustive bfloat16 sweep ---------------------------------------------------------------------------------------
SWEEP_SHAPE = {"8p192": (264, 144), "dma64": (840, 40), "dma256": (264, 256), "reg_auto": (128, 264), "auto_small_m": (264, 128)}


def _sweep(family, tile, dtype, M, N, K):
    f32_out = dtype == F32
    seen = 0
    for case in R.sweep_gelu_cases(M, N, K, dtype):
        outs, chain, _, p = run(family, case, "F2", tile)
        fast = R.CHAINS[chain][2]
        x = case.acc
        want = (case.acc + 0.0).to(F32 if f32_out else BF)          # (a sum that starts at +0 gives +0 for a swept -0)
        assert torch.equal(_bits(p[:, :N].cpu()), _bits(want)), (family, "the saved pre-activation is not the swept value bit for bit")
        c = outs["C"]
        assert torch.isfinite(c).all()
        assert torch.equal(c[x >= 6], x[x >= 6])
        bound = R.sweep_bounds(x, "gelu", fast, f32_out)
        ratio = R.worst_ratio(c, R.gelu64(x), bound)
        print(f"RATIO {family} F2/sweep C {ratio:.3f} [{chain}{'/f32' if f32_out else ''}]")
        assert ratio <= R.GATE, (family, chain, ratio)
        seen += N * K
    assert seen >= R.sweep_values().numel()
    case = R.sweep_grad_case(M, N, K, dtype)
    outs, chain, _, _ = run(family, case, "F4", tile)
    fast = R.CHAINS[chain][2]
    x, c = case.preact_in.double(), outs["C"]
    assert torch.isfinite(c).all()
    bound = R.sweep_bounds(x, "grad", fast, f32_out)
    ratio = R.worst_ratio(c, R.gelu_grad64(x), bound)
    print(f"RATIO {family} F4/sweep C {ratio:.3f} [{chain}{'/f32' if f32_out else ''}]")
    assert ratio <= R.GATE, (family, chain, ratio)


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_sweep(family):
    fam = R.FAMILIES[family]
    M, N = SWEEP_SHAPE.get(family, (264, 136))
    _sweep(family, fam["tile"], fam["dtype"], M, N, 64)


@pytest.mark.parametrize("family", ["pp256", "pp192"])
def test_sweep_persistent(family):
    fam = R.PERSISTENT[family]
    _sweep(family, fam["tile"], BF, _persistent_rows(), fam["N"], 256)


# ---- operand layouts, alpha, exact integers --------------------------------------------------------------------------------
def _variants(family, tile, dtype, M, N, K, persistent=False):
    case = R.random_case(M, N, K, dtype)
    if persistent:      # the forms the persistent kernel serves itself, on a column block of a wider A and a padded B
        for form in ("F1", "F2", "F3"):
            check(family + "/a_off+ldb", case, form, tile, a_off=16, ldb_pad=8)
    else:
        check(family + "/ldb", case, "F4", tile, ldb_pad=8)            # Engine.linear_dgrad with wt: K-major B, padded rows
        n8 = N if N % 8 == 0 else _ceil(N, 24) * 24                    # an MN-major B needs N % 8 == 0 (204 -> 216)
        check(family + "/mn", R.random_case(M, n8, K, dtype), "F4", tile, b_mn=True)      # ... without wt: MN-major B
        check(family + "/a_off", case, "F1", tile, a_off=16)           # cols=: a column block of a wider A, lda > K
        check(family + "/a_off", case, "F4", tile, a_off=16)
    half = R.random_case(M, N, K, dtype, alpha=0.5)
    for form in ("F1", "F2", "F3"):
        check(family + "/alpha", half, form, tile)
    ints = R.integer_case(M, N, K if persistent else 64, dtype)
    for form in ("F1", "F3") + (() if dtype == F32 or persistent else ("F6",)):
        outs, chain, _, _ = run(family + "/int", ints, form, tile)
        assert torch.equal(outs["C"], R.reference(ints, form).C), (family, form, chain)


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_layouts_alpha_and_exact_integers(family):
    fam = R.FAMILIES[family]
    _variants(family, fam["tile"], fam["dtype"], fam["Ms"][0], fam["Ns"][-1], 200)


@pytest.mark.parametrize("family", ["pp256", "pp192"])
def test_layouts_alpha_and_exact_integers_persistent(family):
    fam = R.PERSISTENT[family]
    _variants(family, fam["tile"], BF, _persistent_rows(), fam["N"], 256, persistent=True)
