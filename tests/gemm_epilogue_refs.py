"""Host-side references for the per-element tests of the Linear epilogues of htrvt_gemm (include/htrvt.h: alpha, bias, act,
preact, residual, c_f32; the call sites are Engine.linear_fwd / linear_dgrad): tests/test_gemm_epilogue_refs_cpu.py proves
what is claimed here, tests/test_gemm_epilogue_gpu.py holds every kernel family to it.

Forms (float64 functions of the already rounded operands, reference()):
  F1  C = alpha acc + bias                                   qkv
  F2  pre = alpha acc + bias -> preact,  C = gelu(pre)       fc1 forward (exact-erf GELU)
  F3  C = alpha acc + bias + residual                        proj / fc2 forward
  F4  C = alpha acc gelu'(preact_in)                         fc2 dgrad
  F5  F2 without a saved pre-activation
  F6  F1 with float32 C (c_f32)                              the split-bf16 path's products
  F7r / F7g / F7d   F3 / F2 / F4 with float32 C and float32 residual / preact

Rounding chains.  Three epilogue implementations serve these forms and they do NOT round at the same points (rb = round to
bfloat16, v = alpha acc + bias in float32).  With float32 C no chain rounds at all.

  chain    code                                     F1      F2 / F5                         F3              F4
  acc      gemm8p_impl.h:596-668 (one tile per      rb(v)   preact = rb(v)                  rb(v + res)     rb(v gelu'(x))
           workgroup), gemm8pp_impl.h:303-315               C = rb(gelu(rb(v)))   [624-625]   [630-634,667]   [608-616,667]
           (persistent): from the accumulators
  staged   gemm_dma_impl.h:414-419 stages           s       preact = s            [560]     rb(s + res)     rb(s gelu'(x))
           s = rb(v) in LDS, everything else                C = rb(gelu(s))       [565,618]   [572,618]       [555,618]
           works on s [547-618]
  direct   gemm_common.h:232-255 (gemm_epilogue:    rb(v)   preact = rb(v)        [242]     rb(v + res)     rb(v gelu'(x))
           the register-staged kernel, and the              C = rb(gelu(v)): the            [253-255]       [235-237,255]
           LDS-DMA kernels when C is float32,               UNROUNDED value       [244]
           N or ldc no multiple of 8, or 256 columns:
           gemm_dma_impl.h:988-993)

  acc and staged evaluate GELU / GELU' with the packed polynomials of gemm_common.h:158-172 (gelu_erf_fast2,
  gelu_erf_grad_fast2: |error| < 5.2e-7 / 2.7e-7 as stated there), direct with libm's erff / __expf (gemm_common.h:129-132).

Error model (error_model(): per element, against float64), u = 2^-8:
  e_v      = 2 K 2^-24 |alpha| (|A| |B|^T)  +  2^-22 (|alpha acc| + |bias|)
             (gamma_K of a float32 sum in any order, doubled for a matrix unit that truncates; one float32 multiply-add)
  rnd(y,e) = u (|y| + e)   one bfloat16 rounding of a value within e of y (+ 2^-133, half a bfloat16 denormal step)
  F1       acc / direct: e_v + rnd(v, e_v);  staged: the same (s IS the result)
  F2       d_pre = e_v + rnd(v, e_v) bounds the stored pre-activation; GELU sees a value within d of pre, d = d_pre where
           the chain applies GELU to the rounded value (acc, staged), d = e_v where not (direct):
             e_g = |gelu'(pre)| d + 0.6 d^2 + approx + 2^-22 |gelu(pre)|       (|gelu''| <= 0.8: second-order term 0.6 d^2)
             C:    e_g + rnd(gelu(pre), e_g)
           approx = 5.2e-7 (polynomial) or 2^-22 |pre| (libm: 0.5 x (1 + erff) has an absolute error of 2^-23 in the bracket)
  F3       d = e_v (acc, direct) or e_v + rnd(v, e_v) (staged);  e = d + 2^-22 (|v| + |res|);  C: e + rnd(v + res, e)
  F4       g = gelu'(x), d as in F3;  e = d (|g| + approx) + |v| approx + 2^-22 |v g|;  C: e + rnd(v g, e)
           approx = 2.7e-7 (polynomial) or 2^-22 (libm)
The gate is GATE = 1.0 x this bound on every element -- not the factor 2 of the attention tests: the emulation of a chain
with ONE more bfloat16 rounding of the intermediate reaches only 1.7-1.9 x the bound of GELU' (measured, K <= 512), so a
factor of 2 could not tell a kernel that rounds once too often from one that does not.

emulate() is the float32 host emulation of each chain (float32 torch product, the chain's roundings, the polynomials written
out in float32) with the mutants the CPU test needs; the worst ratios it reaches over the random cases of the GPU file are
in EMULATION_WORST (asserted as a ceiling of 1.0 by the CPU test).

Cases: random_case (A = randn, B = sigma randn with pre-activations spanning about +-4, bias / residual / preact_in =
1.5 randn, all rounded to the operand type, one seed per shape), the exhaustive bfloat16 sweep (sweep_values: every finite
bfloat16 of magnitude <= 8 with denormals and both zeros, and +-{16, 100, 1e4, largest finite}; one-hot A rows so that acc
is exactly the swept value) and exact integer cases (integer_case)."""
import functools
import math
from types import SimpleNamespace

import torch

from attn_refs import assert_guards_intact, guarded, worst_ratio  # noqa: F401  (re-exported for the GPU file)

U = 2.0 ** -8
F32EPS = 2.0 ** -22
TINY = 2.0 ** -133
GATE = 1.0
GELU_FAST_ERR = 5.2e-7            # gemm_common.h:141
GELUGRAD_FAST_ERR = 2.7e-7
SQRT2 = math.sqrt(2.0)
BF = torch.bfloat16

FORMS = ("F1", "F2", "F3", "F4", "F5", "F6", "F7r", "F7g", "F7d")
F32_OUT = {"F6", "F7r", "F7g", "F7d"}
# form -> (act, bias, writes preact, reads residual, reads preact_in)
FORM_SPEC = {"F1": (0, True, False, False, False), "F2": (1, True, True, False, False), "F3": (0, True, False, True, False),
             "F4": (2, False, False, False, True), "F5": (1, True, False, False, False), "F6": (0, True, False, False, False),
             "F7r": (0, True, False, True, False), "F7g": (1, True, True, False, False), "F7d": (2, False, False, False, True)}
# chain -> (the staged value is rounded first, GELU is applied to the rounded pre-activation, packed polynomials)
CHAINS = {"acc": (False, True, True), "staged": (True, True, True), "direct": (False, False, False)}
# worst |emulation - float64| / bound over RANDOM_SHAPES and the sweep, per (chain, form, output); measured on the CPU
EMULATION_WORST = {
    ("acc", "F1", "C"): 0.993, ("acc", "F2", "C"): 0.954, ("acc", "F2", "preact"): 0.993, ("acc", "F3", "C"): 0.993,
    ("acc", "F4", "C"): 0.991, ("acc", "F5", "C"): 0.954, ("acc", "F2/sweep", "C"): 0.967, ("acc", "F4/sweep", "C"): 0.993,
    ("staged", "F1", "C"): 0.993, ("staged", "F2", "C"): 0.954, ("staged", "F2", "preact"): 0.993, ("staged", "F3", "C"): 0.988,
    ("staged", "F4", "C"): 0.963, ("staged", "F5", "C"): 0.954, ("staged", "F2/sweep", "C"): 0.967, ("staged", "F4/sweep", "C"): 0.993,
    ("direct", "F1", "C"): 0.993, ("direct", "F2", "C"): 0.992, ("direct", "F2", "preact"): 0.993, ("direct", "F3", "C"): 0.993,
    ("direct", "F4", "C"): 0.991, ("direct", "F5", "C"): 0.992, ("direct", "F2/sweep", "C"): 0.975, ("direct", "F4/sweep", "C"): 0.993,
    ("direct", "F6", "C"): 0.021, ("direct", "F7r", "C"): 0.023, ("direct", "F7g", "C"): 0.125, ("direct", "F7g", "preact"): 0.021,
    ("direct", "F7d", "C"): 0.194,
    # float32 operands (the register-staged kernel's exact-float32 MFMA): forms F1 .. F5 with float32 C
    ("direct", "F1/f32", "C"): 0.032, ("direct", "F2/f32", "C"): 0.124, ("direct", "F2/f32", "preact"): 0.032,
    ("direct", "F3/f32", "C"): 0.032, ("direct", "F4/f32", "C"): 0.194, ("direct", "F5/f32", "C"): 0.124,
}


def rb(x):
    """round to bfloat16 (nearest even), back in the dtype of x"""
    return x.to(BF).to(x.dtype)


# ---- float64 functions ------------------------------------------------------------------------------------------------
def normal_pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def normal_cdf(x):
    return 0.5 * torch.erfc(-x / SQRT2)           # (erfc: no cancellation in the left tail)


def gelu64(x):
    return x * normal_cdf(x)


def gelu_grad64(x):
    return normal_cdf(x) + x * normal_pdf(x)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def reference(case, form):
    """float64 result of `form` on `case` -> namespace C, preact (None unless the form saves it), v = alpha acc + bias"""
    act, with_bias, _, with_res, with_pre = FORM_SPEC[form]
    acc = case.acc
    v = case.alpha * acc + (case.bias.double() if with_bias and case.bias is not None else 0.0)
    r = SimpleNamespace(v=v, preact=None)
    if act == 1:
        r.preact, r.C = v, gelu64(v)
    elif act == 2:
        r.C = v * gelu_grad64(case.preact_in.double())
    else:
        r.C = v + (case.residual.double() if with_res else 0.0)
    return r


def error_model(case, form, chain, f32_out=None):
    """per-element bounds of the module docstring -> dict output name -> float64 tensor ("C", and "preact" for F2 / F7g)"""
    staged, gelu_rounded, fast = CHAINS[chain]
    if f32_out is None:
        f32_out = form in F32_OUT
    act, with_bias, saves, with_res, _ = FORM_SPEC[form]
    u = 0.0 if f32_out else U
    r = reference(case, form)
    v = r.v

    def rnd(y, e):
        return u * (y.abs() + e) + (TINY if u else 0.0)

    bias_mag = case.bias.double().abs() if with_bias and case.bias is not None else 0.0
    e_v = 2.0 * case.K * 2.0 ** -24 * abs(case.alpha) * case.absacc + F32EPS * ((case.alpha * case.acc).abs() + bias_mag)
    d_round = e_v + rnd(v, e_v)
    out = {}
    if act == 1:
        d = d_round if (gelu_rounded and not f32_out) else e_v
        approx = GELU_FAST_ERR if fast else F32EPS * v.abs()
        e_g = gelu_grad64(v).abs() * d + 0.6 * d * d + approx + F32EPS * r.C.abs()
        out["C"] = e_g + rnd(r.C, e_g)
        if saves:
            out["preact"] = d_round
    elif act == 2:
        d = d_round if (staged and not f32_out) else e_v
        g = gelu_grad64(case.preact_in.double()).abs()
        approx = GELUGRAD_FAST_ERR if fast else F32EPS
        e = d * (g + approx) + v.abs() * approx + F32EPS * r.C.abs()
        out["C"] = e + rnd(r.C, e)
    elif with_res:
        d = d_round if (staged and not f32_out) else e_v
        e = d + F32EPS * (v.abs() + case.residual.double().abs())
        out["C"] = e + rnd(r.C, e)
    else:
        out["C"] = d_round
    return out


# ---- float32 emulation of the chains -----------------------------------------------------------------------------------
_ERFC = (1.986000183e-05, -6.623090474e-04, 7.759703627e-03, -5.296444113e-02, -4.590662242e-01, -1.151119094e+00)


def _erfc_abs(ax):
    """gemm_common.h erfc_abs2 in float32 torch: (a = min(|x|, 4 sqrt 2), erfc(a / sqrt 2) = exp2(a R(a)))"""
    a = ax.clamp(0.0, 5.656854249)
    r = torch.full_like(a, _ERFC[0])
    for c in _ERFC[1:]:
        r = r * a + c
    return a, torch.exp2(a * r)


def gelu_fast(x):
    """gelu_erf_fast2 (float32)"""
    ax = x.abs()
    a, e = _erfc_abs(ax)
    return (x * 0.5 + ax * 0.5) - (a * 0.5) * e


def gelu_grad_fast(x):
    """gelu_erf_grad_fast2 (float32)"""
    _, e = _erfc_abs(x.abs())
    d = torch.copysign(0.5 - 0.5 * e, x)
    pdf = torch.exp2((x * x) * -0.72134752044448170368)
    return (x * 0.39894228040143267794) * pdf + 0.5 + d


def gelu_libm(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def gelu_grad_libm(x):
    return 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440)) + x * 0.39894228040143267794 * torch.exp(-0.5 * x * x)


MUTANTS = ("extra_round", "tanh", "bias_n1", "side_m1", "grad_unrounded")


def emulate(case, form, chain, f32_out=None, mutant=None, tile_rows=256):
    """the chain's arithmetic in float32 -> dict output name -> float32 tensor.  mutant: one of MUTANTS --
    extra_round     one more bfloat16 rounding of the intermediate: of v in front of GELU where the chain has none (direct), of
                    alpha acc in front of the bias where it has (acc, staged) -- F2 / F5; of v, or of alpha acc in front of the bias
                    for the staged chain -- F3; of v, or of the GELU' value for the staged chain -- F4
    tanh            tanh-GELU in place of the erf one
    bias_n1         the bias of column n + 1
    side_m1         residual / preact_in of row m + 1 in the last partial tile of `tile_rows` rows
    grad_unrounded  GELU' at the value before it was rounded to the operand type (case.preact_raw)"""
    staged, gelu_rounded, fast = CHAINS[chain]
    if f32_out is None:
        f32_out = form in F32_OUT
    act, with_bias, saves, with_res, with_pre = FORM_SPEC[form]
    rnd = (lambda y: y) if f32_out else rb
    f = torch.float32
    acc = case.A.to(f) @ case.B.to(f).t()
    v = acc * case.alpha
    if mutant == "extra_round" and not f32_out and ((act == 1 and gelu_rounded) or (with_res and staged)):
        v = rb(v)
    if with_bias and case.bias is not None:
        bias = case.bias.to(f)
        if mutant == "bias_n1":
            bias = torch.roll(bias, -1)
        v = v + bias

    def side(t):
        t = t.to(f)
        if mutant == "side_m1":
            M = t.shape[0]
            first = (M - 1) // tile_rows * tile_rows
            rows = torch.arange(M)
            rows[first:M - 1] += 1
            rows[M - 1] = first - 1 if first > 0 else M - 1      # (no row M: the last row takes the one in front of the tile)
            t = t[rows]
        return t

    s = rnd(v) if staged else v
    out = {}
    if act == 1:
        p = rnd(v)
        x = p if gelu_rounded else v
        if mutant == "extra_round" and not gelu_rounded:
            x = rb(v)
        if mutant == "tanh":
            y = gelu_tanh(x)
        else:
            y = gelu_fast(x) if fast else gelu_libm(x)
        out["C"] = rnd(y)
        if saves:
            out["preact"] = p
    elif act == 2:
        x = side(case.preact_raw if mutant == "grad_unrounded" else case.preact_in)
        g = gelu_grad_fast(x) if fast else gelu_grad_libm(x)
        if mutant == "extra_round" and not f32_out:
            if staged:
                g = rb(g)
            else:
                s = rb(s)
        out["C"] = rnd(s * g)
    elif with_res:
        if mutant == "extra_round" and not f32_out and not staged:
            s = rb(s)
        out["C"] = rnd(s + side(case.residual))
    else:
        out["C"] = rnd(s)
    return out


def mutants_of(form, chain, f32_out=None):
    """the mutants of emulate() that change `form` on `chain`"""
    act, with_bias, _, with_res, with_pre = FORM_SPEC[form]
    if f32_out is None:
        f32_out = form in F32_OUT
    m = []
    if not f32_out and (act in (1, 2) or with_res):
        m.append("extra_round")
    if act == 1:
        m.append("tanh")
    if with_bias:
        m.append("bias_n1")
    if with_res or with_pre:
        m.append("side_m1")
    if with_pre and not f32_out:
        m.append("grad_unrounded")
    return m


# ---- cases ------------------------------------------------------------------------------------------------------------
def _finish(case):
    case.acc = case.A.double() @ case.B.double().t()
    case.absacc = case.A.double().abs() @ case.B.double().abs().t()
    case.M, case.K = case.A.shape
    case.N = case.B.shape[0]
    return case


def case_seed(M, N, K):
    return 7000 + 31 * M + 17 * N + K


@functools.lru_cache(maxsize=4)
def random_case(M, N, K, dtype=BF, alpha=1.0, seed_offset=0):
    """A = randn, B = 1.3 / sqrt(K) / alpha randn (alpha acc ~ N(0, 1.7), with the bias about +-4 at two sigma), bias / residual /
    preact_in = 1.5 randn; A, B and the C-typed side tensors rounded to `dtype`, bias float32.  residual32 / preact32 are the
    float32 side tensors of the F7 forms."""
    g = torch.Generator().manual_seed(case_seed(M, N, K) + seed_offset)
    c = SimpleNamespace(alpha=alpha, dtype=dtype)
    c.A = torch.randn(M, K, generator=g).to(dtype)
    c.B = (torch.randn(N, K, generator=g) * (1.3 / math.sqrt(K) / alpha)).to(dtype)
    c.bias = torch.randn(N, generator=g) * 1.5
    c.residual32 = torch.randn(M, N, generator=g) * 1.5
    c.preact_raw = torch.randn(M, N, generator=g) * 1.5
    c.residual = c.residual32.to(dtype)
    c.preact_in = c.preact_raw.to(dtype)
    return _finish(c)


def as_f32_sides(case):
    """the same case with the float32 side tensors in the C-typed slots (forms F7r / F7d)"""
    c = SimpleNamespace(**vars(case))
    c.residual, c.preact_in = case.residual32, case.preact_raw
    return c


@functools.lru_cache(maxsize=None)
def sweep_values():
    """every finite bfloat16 of magnitude <= 8 (denormals and both zeros included) and +-{16, 100, 1e4, largest finite}, as a
    bfloat16 vector (33 290 values)"""
    bits = torch.arange(0, 0x4100 + 1, dtype=torch.int32)                       # 0x4100 = 8.0
    extra = torch.tensor([16.0, 100.0, 1e4, 3.3895313892515355e38]).to(BF).view(torch.int16).to(torch.int32)
    pos = torch.cat([bits, extra])
    return torch.cat([pos, pos - 0x8000]).to(torch.int16).view(BF)        # (the sign bit, in int16 two's complement)


def sweep_gelu_cases(M, N, K, dtype=BF):
    """F2 on the sweep: one-hot rows A[m][m % K] = 1 and B holding the swept values give acc[m][n] = B[n][m % K] exactly
    (alpha = 1, no bias); N K values fit one launch, so the sweep takes ceil(33 290 / (N K)) cases.  A sum that starts at +0
    returns +0 for a swept -0: case.acc is that exact float64 value."""
    vals = sweep_values()
    per = N * K
    cases = []
    for lo in range(0, vals.numel(), per):
        chunk = vals[lo:lo + per]
        b = torch.zeros(per, dtype=BF)
        b[:chunk.numel()] = chunk
        c = SimpleNamespace(alpha=1.0, dtype=dtype, bias=None)
        c.A = torch.zeros(M, K, dtype=dtype)
        c.A[torch.arange(M), torch.arange(M) % K] = 1.0
        c.B = b.reshape(N, K).to(dtype)
        cases.append(_finish(c))
    return cases


def sweep_grad_case(M, N, K, dtype=BF):
    """F4 on the sweep: acc == 1 (one-hot A rows, B of ones), preact_in[m][n] = sweep[(m N + n) % 33 290]"""
    vals = sweep_values()
    assert M * N >= vals.numel()
    c = SimpleNamespace(alpha=1.0, dtype=dtype, bias=None)
    c.A = torch.zeros(M, K, dtype=dtype)
    c.A[torch.arange(M), torch.arange(M) % K] = 1.0
    c.B = torch.ones(N, K, dtype=dtype)
    c.preact_in = vals[torch.arange(M * N) % vals.numel()].reshape(M, N).to(dtype)
    c.preact_raw = c.preact_in
    return _finish(c)


def sweep_bounds(x64, which, fast, f32_out=False):
    """the sweep's own gates: u |gelu64| + approximation (F2), u |gelu'64| + approximation (F4, acc == 1); a float32 output has
    the rounding of its last float32 operation, 2^-22 |result|, in place of the bfloat16 one"""
    u = F32EPS if f32_out else U
    if which == "gelu":
        return u * gelu64(x64).abs() + (GELU_FAST_ERR if fast else F32EPS * x64.abs()) + TINY
    return u * gelu_grad64(x64).abs() + (GELUGRAD_FAST_ERR if fast else F32EPS)


def integer_case(M, N, K, dtype=BF, seed=0):
    """exact in every chain: A in {-1, 0, 1}, B in [-2, 2], bias in [-20, 20], residual in [-30, 30], every intermediate an
    integer below 256 in magnitude (asserted), i.e. a bfloat16 value"""
    g = torch.Generator().manual_seed(9000 + seed + 31 * M + 17 * N + K)
    c = SimpleNamespace(alpha=1.0, dtype=dtype)
    c.A = torch.randint(-1, 2, (M, K), generator=g).to(dtype)
    c.B = torch.randint(-2, 3, (N, K), generator=g).to(dtype)
    c.bias = torch.randint(-20, 21, (N,), generator=g).float()
    c.residual = torch.randint(-30, 31, (M, N), generator=g).to(dtype)
    c.residual32 = c.residual.float()
    _finish(c)
    assert float((c.acc + c.bias.double()).abs().max()) + 30 < 256
    return c


# ---- the shapes of the GPU file (tests/test_gemm_epilogue_gpu.py builds its case lists from this table) ----------------
KS = (64, 200, 256)
# family -> selector, operand type, M list, N list, K list, the chain of its bfloat16-C forms when it serves them itself
FAMILIES = {
    "8p256":        dict(tile=10, dtype=BF, Ms=(129, 257, 520), Ns=(8, 264), Ks=KS, chain="acc"),
    "8p192":        dict(tile=11, dtype=BF, Ms=(129, 257, 520), Ns=(24, 204), Ks=KS, chain="acc"),
    "dma192":       dict(tile=3, dtype=BF, Ms=(129, 257, 520), Ns=(200, 264, 392), Ks=KS, chain="staged"),
    "dma192_lw":    dict(tile=4, dtype=BF, Ms=(129, 257, 520), Ns=(200, 264, 392), Ks=KS, chain="staged"),
    "dma128_s2":    dict(tile=7, dtype=BF, Ms=(129, 257, 520), Ns=(136,), Ks=KS, chain="staged"),
    "dma128_s3":    dict(tile=8, dtype=BF, Ms=(129, 257, 520), Ns=(136,), Ks=KS, chain="staged"),
    "dma64":        dict(tile=0, dtype=BF, Ms=(257,), Ns=(40,), Ks=KS, chain="staged"),
    "dma256":       dict(tile=6, dtype=BF, Ms=(257,), Ns=(256,), Ks=KS, chain="direct"),
    "auto_small_m": dict(tile=0, dtype=BF, Ms=(520,), Ns=(384, 768), Ks=KS, chain="staged"),
    "auto_decline": dict(tile=0, dtype=BF, Ms=(520,), Ns=(776,), Ks=KS, chain="staged"),
    "reg_auto":     dict(tile=0, dtype=BF, Ms=(37, 128), Ns=(40, 200), Ks=KS, chain="direct"),
    "reg_bf16":     dict(tile=1, dtype=BF, Ms=(257,), Ns=(40, 200), Ks=KS, chain="direct"),
    "reg_f32":      dict(tile=0, dtype=torch.float32, Ms=(37, 257), Ns=(40, 200), Ks=KS, chain="direct"),
}
# the persistent kernels: M = 256 t + 1 with t from the device's CU count (the GPU file), N with five column tiles
PERSISTENT = {"pp256": dict(tile=14, N=1032), "pp192": dict(tile=15, N=780), "pp_auto_1032": dict(tile=0, N=1032),
              "pp_auto_780": dict(tile=0, N=780)}
PERSISTENT_KS = (256, 384)


def random_shapes():
    """every (M, N, K, dtype) of a random case of the GPU file but the persistent ones (whose M depends on the device)"""
    seen = []
    for fam in FAMILIES.values():
        for M in fam["Ms"]:
            for N in fam["Ns"]:
                for K in fam["Ks"]:
                    if (M, N, K, fam["dtype"]) not in seen:
                        seen.append((M, N, K, fam["dtype"]))
    return seen
