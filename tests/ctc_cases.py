"""Seeded inputs for the CTC loss tests (tests/test_ctc_cases_cpu.py, tests/test_ctc_gpu.py): plain numpy, no device.

A case is (name, logits [B,T,C] float32, targets int32 (concatenated), lengths int32 [B], max_target_len or None).
`max_target_len` is the bound the launch is given when it is larger than the batch needs (what a captured training
step does); None = the batch's own maximum.  Every case keeps sum_b T * (2 L_b + 1) <= 250 000, so the pure-Python
float64 oracle (oracle.htrvt_oracle.ctc_loss) takes about a second on it.

The shapes follow the dispatch of csrc/ctc.hip: K = ceil((2 * max_target_len + 1) / 64) states per lane for K = 1..4,
one workgroup per sample (ctc_kernel) beyond, with its own S <= 256 / S > 256 branches."""
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name logits targets lengths max_target_len")

NLL_RTOL = 1e-5       # |nll - ref| <= NLL_RTOL * max(1, max|ref|)           (tests/test_model_gpu.py, known answers)
GRAD_RTOL = 4e-3      # max|grad - ref| < GRAD_RTOL * max|ref grad|


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _i32(v):
    return np.asarray(v, dtype=np.int32)


def repeats(lab):
    """adjacent equal label pairs: a blank must separate them, so T >= L + repeats(lab)"""
    lab = np.asarray(lab)
    return int((lab[1:] == lab[:-1]).sum()) if lab.size > 1 else 0


def split(targets, lengths):
    out, off = [], 0
    for L in np.asarray(lengths).tolist():
        out.append(np.asarray(targets[off:off + L], dtype=np.int64))
        off += L
    return out


def bound_of(case):
    return int(case.max_target_len if case.max_target_len is not None else (case.lengths.max() if case.lengths.size else 0))


def lane_states(case):
    """K of the register-resident instance the launch takes; 0 = ctc_kernel"""
    smax = 2 * bound_of(case) + 1
    return (smax + 63) // 64 if smax <= 256 else 0


def cost(case):
    return int(sum(case.logits.shape[1] * (2 * int(L) + 1) for L in case.lengths))


def forced_path(lab, T):
    """the only alignment of `lab` over T = L + repeats(lab) frames: every label once, a blank between equal
    neighbours (no label at all: blanks only, for any T)"""
    path = []
    for i, v in enumerate(np.asarray(lab).tolist()):
        if i > 0 and lab[i - 1] == v:
            path.append(0)
        path.append(int(v))
    if not path:
        path = [0] * T
    assert len(path) == T
    return np.asarray(path, dtype=np.int64)


def closed_form(case):
    """exact nll / gradient of a single-alignment case in float64: nll = -sum_t logp[t, path[t]],
    grad = (softmax - onehot(path)) / B; an infeasible sample (T < L + repeats) has zero nll and zero gradient"""
    x = case.logits.astype(np.float64)
    B, T, C = x.shape
    mx = x.max(axis=2, keepdims=True)
    lp = x - mx - np.log(np.exp(x - mx).sum(axis=2, keepdims=True))
    nll, grad = np.zeros(B), np.zeros_like(x)
    for b, lab in enumerate(split(case.targets, case.lengths)):
        need = len(lab) + repeats(lab)
        if need > T:
            continue
        assert need == T or len(lab) == 0, "not a single-alignment sample"
        path = forced_path(lab, T)
        nll[b] = -lp[b, np.arange(T), path].sum()
        grad[b] = np.exp(lp[b])
        grad[b, np.arange(T), path] -= 1.0
    return nll, grad / B


def _labels(rng, L, C):
    return rng.integers(1, C, size=L)


def _plant_repeat(lab, k):
    lab[k + 1] = lab[k]


def _case(name, logits, labs, bound=None):
    lengths = _i32([len(l) for l in labs])
    targets = _i32(np.concatenate([np.asarray(l, dtype=np.int64) for l in labs]) if labs else [])
    c = Case(name, np.ascontiguousarray(logits, dtype=np.float32), targets, lengths, bound)
    assert cost(c) <= 250_000, (name, cost(c))
    return c


def _boundary(Lmax, T, tag):
    name = f"{tag}_L{Lmax}_T{T}"
    rng = _rng(name)
    C = 80
    labs = [_labels(rng, L, C) for L in (Lmax, 0, 1, Lmax // 2 + 1)]
    _plant_repeat(labs[0], Lmax // 3)
    assert Lmax + repeats(labs[0]) <= T
    return _case(name, rng.normal(0.0, 2.0, (4, T, C)), labs)


def boundary_cases():
    """the batch maximum on either side of every K switch: S = 63 | 65, 127 | 129, 191 | 193, 255 (the last lane of K = 4
    half active); at 32 / 64 / 96 labels the last state sits alone in a fresh lane.  T = Lmax + 13 is tight: little weight
    ends in the final blank there, so a lost last state can hide (tests/test_ctc_cases_cpu.py measures it); T = 256 is
    loose, and every K has such a case"""
    out = [_boundary(L, L + 13, "edge") for L in (31, 32, 63, 64, 95, 96, 127)]
    out += [_boundary(L, 256, "edge") for L in (31, 32, 64, 95, 127)]
    return out


BOUNDS = (31, 64, 127, 130)


def bound_cases():
    """one batch launched under its own maximum and under larger bounds: K = 1, 3, 4 and the S <= 256 branch of ctc_kernel.
    The four cases share their arrays (and their oracle values)."""
    rng = _rng("bound")
    C, T = 80, 64
    labs = [_labels(rng, L, C) for L in (20, 7, 0, 31)]
    logits = rng.normal(0.0, 2.0, (4, T, C))
    base = _case("bound_31", logits, labs, 31)
    return [base] + [Case(f"bound_{m}", base.logits, base.targets, base.lengths, m) for m in BOUNDS[1:]]


def _single(L, bound=None):
    name = f"single_L{L}"
    rng = _rng(name)
    C = 20
    lab = _labels(rng, L, C)
    if L >= 2:
        _plant_repeat(lab, L // 2 - 1 if L > 2 else 0)
    T = L + repeats(lab)
    labs = [lab]
    if L >= 5:                         # the same labels with one more repeat: T = L + r - 1, infeasible
        bad = lab.copy()
        for k in rng.permutation(L - 1):
            trial = lab.copy()
            _plant_repeat(trial, int(k))
            if repeats(trial) == repeats(lab) + 1:
                bad = trial
                break
        assert len(bad) + repeats(bad) == T + 1
        labs.append(bad)
    labs.append(np.zeros(0, dtype=np.int64))          # no label: the all-blank path is the only one, for any T
    return _case(name, rng.normal(0.0, 2.0, (len(labs), T, C)), labs, bound)


def single_alignment_cases():
    """T = L + repeats: exactly one alignment, almost every alpha / beta is -inf; the answer is closed_form()"""
    return [_single(L) for L in (1, 5, 32, 64, 127)] + [_single(130, 130)]


def short_cases():
    """T = 1..6: the emission prefetch clamps at both ends, the PF-unrolled loop breaks in its first trip.  C = 2 leaves
    the label 1 only: every neighbouring pair is a repeat"""
    out = []
    for C in (2, 65):
        for T in range(1, 7):
            name = f"short_T{T}_C{C}"
            rng = _rng(name)
            lens = [0, 1, (T + 1) // 2, T, T + 1, 2]
            labs = [_labels(rng, L, C) for L in lens]
            out.append(_case(name, rng.normal(0.0, 2.0, (len(labs), T, C)), labs))
    return out


def class_cases():
    """class counts around the 64-lane stride of the per-row loops; C = 300 on ctc_kernel walks head[c] for c >= 256"""
    out = []
    for C in (2, 63, 64, 65, 129):
        name = f"classes_C{C}"
        rng = _rng(name)
        labs = [_labels(rng, L, C) for L in (40, 0, 17)]
        out.append(_case(name, rng.normal(0.0, 2.0, (3, 90, C)), labs))
    rng = _rng("classes_C300")
    labs = [_labels(rng, L, 300) for L in (128, 60)]
    out.append(_case("classes_C300", rng.normal(0.0, 2.0, (2, 140, 300)), labs))
    return out


def long_cases():
    """ctc_kernel: three states per thread (S = 521); labels that occur more than four times in a sample (the `rest`
    walk of the register-cached class lists, S <= 256 branch, and long lists in the S > 256 branch); a launch in which
    every sample is infeasible"""
    out = []
    rng = _rng("long_S521")
    labs = [_labels(rng, L, 40) for L in (260, 128, 0)]
    out.append(_case("long_S521", rng.normal(0.0, 2.0, (3, 300, 40)), labs))
    rng = _rng("long_three_labels")
    labs = [_labels(rng, L, 4) for L in (130, 100)]
    T = max(len(l) + repeats(l) for l in labs) + 40
    out.append(_case("long_three_labels", rng.normal(0.0, 2.0, (2, T, 4)), labs))
    rng = _rng("long_infeasible")
    labs = [_labels(rng, L, 40) for L in (130, 129)]
    out.append(_case("long_infeasible", rng.normal(0.0, 2.0, (2, 128, 40)), labs))
    return out


def _alignment(rng, lab, T):
    """a valid alignment of `lab` over T frames: the forced path, then random frames doubled"""
    path = forced_path(lab, len(lab) + repeats(lab)).tolist() if len(lab) else [0]
    while len(path) < T:
        k = int(rng.integers(0, len(path)))
        path.insert(k, path[k])
    return np.asarray(path, dtype=np.int64)


def _peaked(name, lens, T, C):
    rng = _rng(name)
    labs = [_labels(rng, L, C) for L in lens]
    logits = rng.normal(0.0, 1.0, (len(lens), T, C))
    for b, lab in enumerate(labs):
        logits[b, np.arange(T), _alignment(rng, lab, T)] += 12.0
    return _case(name, logits, labs)


def peaked_cases():
    """normal(0, 1) + 12 on the classes of one valid alignment: nll near 0, occupancies near 0 or 1"""
    return [_peaked("peaked_fast", (50, 20, 0, 33), 120, 80), _peaked("peaked_long", (140, 130), 200, 40)]


MASKED_CLASSES = (5, 17, 79)


def masked_cases():
    """-inf on classes that no target holds: nll and gradient stay finite, the gradient is exactly 0 there"""
    rng = _rng("masked")
    C = 80
    allowed = np.setdiff1d(np.arange(1, C), MASKED_CLASSES)
    labs = [rng.choice(allowed, size=L) for L in (30, 12, 0, 25)]
    logits = rng.normal(0.0, 2.0, (4, 60, C))
    logits[:, :, list(MASKED_CLASSES)] = -np.inf
    return [_case("masked", logits, labs)]


def all_cases():
    cases = (boundary_cases() + bound_cases() + single_alignment_cases() + short_cases() + class_cases() + long_cases()
             + peaked_cases() + masked_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = {c.name: c for c in all_cases()}


def oracle_key(name):
    """the bound cases are one batch: one oracle evaluation serves all four"""
    return "bound_31" if name.startswith("bound_") else name


def one_per_k():
    """a ragged case (L = 0 included) for every K, and one for each branch of ctc_kernel"""
    return {1: "bound_31", 2: "edge_L63_T76", 3: "edge_L95_T108", 4: "edge_L127_T140", "wg_le256": "bound_130",
            "wg_gt256": "long_S521"}


def aten_ctc(case, dtype):
    """log_softmax + ATen's CPU CTC (reduction none, zero_infinity) and the gradient of the batch mean w.r.t. the logits,
    evaluated in `dtype`.  ATen's backward turns a -inf log-probability into NaN, so masked classes are taken out of the
    problem first (the softmax over the rest is the same) and get the gradient 0 they have."""
    import torch
    x = case.logits
    keep = np.nonzero(np.isfinite(x).all(axis=(0, 1)))[0]
    remap = np.full(x.shape[2], -1, dtype=np.int64)
    remap[keep] = np.arange(keep.size)
    tg = remap[case.targets.astype(np.int64)]
    assert (tg >= 0).all()
    xt = torch.tensor(x[:, :, keep], dtype=dtype, requires_grad=True)
    B, T, _ = xt.shape
    lp = xt.permute(1, 0, 2).log_softmax(2)
    nll = torch.nn.functional.ctc_loss(lp, torch.from_numpy(tg), torch.full((B,), T, dtype=torch.int64),
                                       torch.from_numpy(case.lengths.astype(np.int64)), blank=0, reduction="none",
                                       zero_infinity=True)
    nll.mean().backward()
    grad = np.zeros(x.shape, dtype=np.float64)
    grad[:, :, keep] = xt.grad.double().numpy()
    return nll.detach().double().numpy(), grad


def errors(nll, grad, ref_nll, ref_grad):
    """(nll error / its bound, gradient error / its bound): inside the project's bounds when both are <= 1 (< 1)"""
    e_n = np.abs(np.asarray(nll, dtype=np.float64) - ref_nll).max() / (NLL_RTOL * max(1.0, np.abs(ref_nll).max()))
    gmax = np.abs(ref_grad).max()
    d = np.abs(np.asarray(grad, dtype=np.float64) - ref_grad).max()
    e_g = d / (GRAD_RTOL * gmax) if gmax > 0 else (0.0 if d == 0 else np.inf)
    return float(e_n), float(e_g)


_REF = {}


def reference(name):
    """(nll [B], grad [B,T,C]) of the float64 oracle, evaluated once per batch of inputs"""
    key = oracle_key(name)
    if key not in _REF:
        from oracle import htrvt_oracle as O
        c = CASES[key]
        nll, _, grad = O.ctc_loss(c.logits, c.targets, c.lengths)
        nll.setflags(write=False)
        grad.setflags(write=False)
        _REF[key] = (nll, grad)
    return _REF[key]


MUTANTS = ("skip_lost_at_lane_edge", "skip_between_equal_labels", "last_state_dropped", "last_label_state_dropped")


def sample_nll(logits, lab, mutant=None, K=4):
    """the oracle's alpha recursion for one sample, [T,C] float64 logits, vectorised over the states, with one of the
    mistakes a lane-per-K-states kernel can make:
      skip_lost_at_lane_edge     the s-2 -> s transition is lost where s-2 lies in the previous lane (s % K < 2)
      skip_between_equal_labels  the s-2 -> s transition is taken between equal labels too
      last_state_dropped         the final blank is left out of the log-likelihood
      last_label_state_dropped   the final label is left out of the log-likelihood"""
    x = np.asarray(logits, dtype=np.float64)
    T = x.shape[0]
    mx = x.max(axis=1, keepdims=True)
    lp = x - mx - np.log(np.exp(x - mx).sum(axis=1, keepdims=True))
    L = len(lab)
    S = 2 * L + 1
    ext = np.zeros(S, dtype=np.int64)
    ext[1::2] = lab
    s = np.arange(S)
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    if mutant == "skip_lost_at_lane_edge":
        skip &= (s % K) >= 2
    elif mutant == "skip_between_equal_labels":
        skip[2:] = ext[2:] != 0
    em = lp[:, ext]
    alpha = np.full(S, -np.inf)
    alpha[:2] = em[0, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, T):
            a1 = np.concatenate([[-np.inf], alpha[:-1]])
            a2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], alpha[:-2]]), -np.inf)
            m = np.maximum(alpha, np.maximum(a1, a2))
            mm = np.where(np.isneginf(m), 0.0, m)
            alpha = mm + np.log(np.exp(alpha - mm) + np.exp(a1 - mm) + np.exp(a2 - mm)) + em[t]
    last = -np.inf if mutant == "last_state_dropped" else alpha[S - 1]
    label = alpha[S - 2] if S > 1 and mutant != "last_label_state_dropped" else -np.inf
    ll = np.logaddexp(last, label)
    return -ll if ll != -np.inf else 0.0
