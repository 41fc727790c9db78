"""htrvt_ctc_loss and htrvt_ctc_greedy_decode (csrc/ctc.hip, csrc/train_aux.hip) at their dispatch edges.

The loss: every case of tests/ctc_cases.py through htrvt_amd.ctc_forward_backward against the float64 oracle
(oracle.htrvt_oracle.ctc_loss; tests/test_ctc_cases_cpu.py shows that it equals the closed form on the
single-alignment cases and ATen's float64 CTC everywhere), under the bounds of test_ctc_kernel_known_answers:
    |nll - ref| <= 1e-5 * max(1, max|ref|),  max|grad - ref| < 4e-3 * max|ref grad|,  exact zeros for infeasible samples.
ATen's float32 CPU CTC is inside both bounds on every case (checked without a device), so a miss is the kernel's.
Every comparison prints the kernel's error beside ATen's, each as a fraction of its bound (`pytest -s`).  Then the
properties the callers rely on: the same nll bits without the gradient, grad_scale as one exact multiply, the same bits
on every run and whatever the nll / grad / workspace buffers held before, refusals that launch nothing.

The decode: first-maximum arg-max, repeat / blank / ncharacter rules, T at the thread-count switches and at the limit
of 16384 frames (more than 64 KB of dynamic LDS above 8192).

Outside the kernels' contract and not tested: NaN logits, labels outside [1, C).

Measured on an MI355X, error as a fraction of its bound, kernel / ATen's float32 CPU CTC on the same inputs (worst case
of each group; every case is in the message of the commit that added this file):

  cases                         nll              gradient
  edge, T = Lmax + 13           0.030 / 0.035    0.127 / 0.155
  edge, T = 256                 0.047 / 0.062    0.259 / 0.311
  bound 31 / 64 / 127 (K)       0.013 / 0.011    0.021 / 0.034     (the same figures under K = 1, 3 and 4)
  bound 130 (ctc_kernel)        0.011 / 0.011    0.031 / 0.034
  single alignment              0.045 / 0.024    0.085 / 0.065
  short T, class counts         0.020 / 0.020    0.078 / 0.075
  long targets                  0.040 / 0.040    0.214 / 0.217
  peaked (|nll| < 1: absolute)  0.535 / 0.155    0.035 / 0.0001
  masked classes                0.011 / 0.032    0.019 / 0.040"""
import numpy as np
import pytest
import torch

import ctc_cases as CC
from oracle import htrvt_oracle as O

pytestmark = pytest.mark.gpu

NAMES = list(CC.CASES)
PER_K = list(CC.one_per_k().values())


@pytest.fixture(scope="module")
def ref():
    """the float64 oracle of a case, evaluated once and shared (read-only)"""
    return CC.reference


def _api():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ctc import ctc_forward_backward, stage_targets
    from htrvt_amd.ops import ptr, stream
    return lib, check, ptr, stream, ctc_forward_backward, stage_targets


def _run(case, **kw):
    """through the wrapper; a launch bound larger than the batch's own maximum goes in through `staged`, as GraphedStep
    passes its capture bound"""
    _, _, _, _, fb, stage = _api()
    logits = torch.from_numpy(case.logits).cuda()
    staged = None
    if case.max_target_len is not None:
        tg, tl, off, own = stage(case.targets, case.lengths, logits.device)
        assert own <= case.max_target_len
        staged = (tg, tl, off, int(case.max_target_len))
    return fb(logits, case.targets, case.lengths, staged=staged, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_ctc_matches_the_float64_oracle(ref, name):
    case = CC.CASES[name]
    ref_nll, ref_grad = ref(name)
    nll, grad = _run(case)
    nll_h, grad_h = nll.cpu().numpy(), grad.cpu().numpy()
    e_n, e_g = CC.errors(nll_h, grad_h, ref_nll, ref_grad)
    a_n, a_g = CC.errors(*CC.aten_ctc(case, torch.float32), ref_nll, ref_grad)
    print(f"\nTABLE {name:18s} K={CC.lane_states(case)} B,T,C={case.logits.shape} max|nll| {np.abs(ref_nll).max():8.2f}  "
          f"nll err/bound kernel {e_n:.4f} ATen {a_n:.4f}   grad err/bound kernel {e_g:.4f} ATen {a_g:.4f}")
    assert np.isfinite(nll_h).all() and np.isfinite(grad_h).all()
    assert e_n <= 1.0, f"nll off by {e_n:.3f} of 1e-5 * max(1, max|ref|) (ATen float32: {a_n:.3f})"
    assert e_g < 1.0, f"gradient off by {e_g:.3f} of 4e-3 * max|ref grad| (ATen float32: {a_g:.3f})"
    for b in np.nonzero(ref_nll == 0)[0]:          # infeasible: zero loss AND zero gradient (zero_infinity)
        assert nll_h[b] == 0.0 and not grad_h[b].any()
    if name == "masked":
        assert not grad_h[:, :, list(CC.MASKED_CLASSES)].any()
    if name.startswith("single_"):                 # the closed form itself, not only the oracle that equals it
        c_nll, c_grad = CC.closed_form(case)
        e_n, e_g = CC.errors(nll_h, grad_h, c_nll, c_grad)
        assert e_n <= 1.0 and e_g < 1.0
        assert (ref_nll == 0).sum() == (1 if case.lengths[0] >= 5 else 0)


@pytest.mark.parametrize("name", PER_K)
def test_ctc_without_gradient_and_twice(name):
    """want_grad=False (one sweep direction on the register path) returns None and the nll bits of the gradient call;
    a second call returns the bits of the first"""
    case = CC.CASES[name]
    nll, grad = _run(case)
    nll0, none = _run(case, want_grad=False)
    assert none is None and torch.equal(nll0, nll)
    nll2, grad2 = _run(case)
    assert torch.equal(nll2, nll) and torch.equal(grad2, grad)


def test_ctc_grad_scale_is_one_exact_multiply():
    """the data-parallel trainer passes 1 / world: (softmax - occupancy) * (grad_scale / B), a power of two here"""
    case = CC.CASES["edge_L63_T76"]
    assert case.logits.shape[0] == 4
    nll, grad = _run(case)
    nll_h, grad_h = _run(case, grad_scale=0.5)
    assert torch.equal(nll_h, nll) and torch.equal(grad_h, grad * 0.5)
    assert grad.abs().max() > 0 and (grad.abs()[grad != 0] > 1e-30).all()      # no subnormal was halved


@pytest.mark.parametrize("name", PER_K)
def test_ctc_reads_nothing_it_has_not_written(name):
    """the wrapper hands the kernels torch.empty memory: with nll, grad and the workspace full of NaN, then full of
    zeros, the C entry point returns the same bits, none of them NaN"""
    lib, check, ptr, stream, _, stage = _api()
    case = CC.CASES[name]
    logits = torch.from_numpy(case.logits).cuda()
    B, T, C = logits.shape
    tg, tl, off, _ = stage(case.targets, case.lengths, logits.device)
    bound = CC.bound_of(case)
    nws = lib.htrvt_ctc_workspace_floats(B, T, bound)
    outs = []
    for fill in (float("nan"), 0.0):
        nll = torch.full((B,), fill, device="cuda")
        grad = torch.full((B, T, C), fill, device="cuda")
        ws = torch.full((nws,), fill, device="cuda")
        check(lib.htrvt_ctc_loss(ptr(logits), ptr(tg), ptr(tl), ptr(off), ptr(nll), ptr(grad), ptr(ws), B, T, C, bound, 1.0,
                                 stream()), "ctc_loss")
        torch.cuda.synchronize()
        outs.append((nll, grad))
    (n0, g0), (n1, g1) = outs
    assert not torch.isnan(n0).any() and not torch.isnan(g0).any()
    assert torch.equal(n0, n1) and torch.equal(g0, g1)
    n2, g2 = _run(case)
    assert torch.equal(n0, n2) and torch.equal(g0, g2)


def test_ctc_refuses_what_it_cannot_launch_without_launching():
    lib, _, ptr, stream, _, _ = _api()
    # ctc_kernel keeps lse [T] + six state arrays + the class heads in LDS: (14000 + 6 * 257 + 4 + 8) * 4 B > 60 KB
    B, T, C, L = 1, 14000, 4, 128
    logits = torch.zeros(B, T, C, device="cuda")
    tg = torch.ones(L, dtype=torch.int32, device="cuda")
    tl = torch.tensor([L], dtype=torch.int32, device="cuda")
    off = torch.zeros(1, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), 7.0, device="cuda")
    grad = torch.full((B, T, C), 7.0, device="cuda")
    ws = torch.full((lib.htrvt_ctc_workspace_floats(B, T, L),), 7.0, device="cuda")
    args = (ptr(logits), ptr(tg), ptr(tl), ptr(off), ptr(nll), ptr(grad), ptr(ws))
    assert lib.htrvt_ctc_loss(*args, B, T, C, L, 1.0, stream()) != 0
    assert b"too large for LDS" in lib.htrvt_last_error()
    for shape in ((B, 0, C), (B, T, 0), (0, T, C)):
        assert lib.htrvt_ctc_loss(*args, *shape, L, 1.0, stream()) != 0
        assert b"bad shape" in lib.htrvt_last_error()
    assert lib.htrvt_ctc_loss(*args, B, T, C, -1, 1.0, stream()) != 0
    torch.cuda.synchronize()
    assert (nll == 7).all() and (grad == 7).all() and (ws == 7).all()


def test_ctc_autograd_wrapper_scales_the_saved_gradient(ref):
    import htrvt_amd
    case = CC.CASES["edge_L32_T45"]
    nll, grad = _run(case)
    x = torch.from_numpy(case.logits).cuda().requires_grad_(True)
    loss = htrvt_amd.ctc_loss(x, case.targets, case.lengths)
    (loss * 3).backward()
    assert torch.equal(loss.detach(), nll.mean()) and torch.equal(x.grad, grad * 3)
    assert abs(loss.item() - ref(case.name)[0].mean()) <= 1e-5 * ref(case.name)[0].max()


# ====================================================================== greedy decode
def _decode_ref(logits, ncharacter=None):
    """O.greedy_decode (arg-max, first maximum; repeats collapsed; blanks dropped), then the converter's cut-off: an index
    >= ncharacter is dropped AFTER it has separated its neighbours (utils.py:80 compares with t[i - 1], kept or not)"""
    seqs = O.greedy_decode(logits)
    if ncharacter is not None:
        seqs = [[v for v in s if v < ncharacter] for s in seqs]
    return seqs


def _decode_both(logits, ncharacter=None, pad=0):
    """through the wrapper and through the C entry point (row stride C + pad, sentinel-filled outputs): both equal the
    reference, the wrapper's tail past `lens` is 0, the entry point's is untouched"""
    lib, check, ptr, stream, _, _ = _api()
    from htrvt_amd.ctc import greedy_decode
    B, T, C = logits.shape
    want = _decode_ref(logits, ncharacter)
    idx, lens = greedy_decode(torch.from_numpy(logits).cuda(), ncharacter=ncharacter)
    buf = torch.full((B, T, C + pad), float("inf"), device="cuda")      # a read past C would win every arg-max
    buf[:, :, :C] = torch.from_numpy(logits).cuda()
    idx2 = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    lens2 = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    check(lib.htrvt_ctc_greedy_decode(ptr(buf), B, T, C, C + pad, C if ncharacter is None else ncharacter, ptr(idx2), ptr(lens2),
                                      stream()), "ctc_greedy_decode")
    idx, lens, idx2, lens2 = idx.cpu().numpy(), lens.cpu().numpy(), idx2.cpu().numpy(), lens2.cpu().numpy()
    assert lens.tolist() == [len(s) for s in want] and lens2.tolist() == lens.tolist()
    for b, s in enumerate(want):
        assert idx[b, :len(s)].tolist() == s and idx2[b, :len(s)].tolist() == s
        assert not idx[b, len(s):].any() and (idx2[b, len(s):] == -7).all()
    return want


def _frames(am, C):
    """logits whose arg-max per frame is `am` [B,T]"""
    x = np.zeros(am.shape + (C,), dtype=np.float32)
    np.put_along_axis(x, np.asarray(am)[..., None], 1.0, axis=2)
    return x


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1023, 1024, 1025])
def test_greedy_decode_at_the_thread_count_switches(T):
    rng = np.random.default_rng(T)
    B, C = 3, 7
    logits = rng.standard_normal((B, T, C)).astype(np.float32)
    logits[1, :, 0] += 1.0
    logits[2] = _frames(rng.integers(0, 3, size=(1, T)), C)[0]           # long runs of repeats and blanks
    _decode_both(logits)
    _decode_both(logits, ncharacter=4)
    _decode_both(logits, pad=5)


def test_greedy_decode_ties_and_empty_rows():
    C = 7
    x = np.zeros((3, 6, C), dtype=np.float32)
    x[0, 0, [2, 5]] = 3.0                       # tie between 2 and 5: the first
    x[0, 1, [0, 4]] = 3.0                       # tie with the blank: the blank
    x[0, 2, :] = 1.5                            # all equal: the blank
    x[0, 3, :] = -np.inf                        # nothing is greater than row[0]: the blank
    x[0, 4, [6]] = 1.0
    x[0, 5, [3, 6]] = 2.0                       # 3 before 6: no repeat of frame 4
    x[1] = -np.inf                              # an all -inf sample decodes to nothing
    x[2, :, 0] = 1.0                            # an all-blank sample
    want = _decode_both(x)
    assert want == [[2, 6, 3], [], []]
    _decode_both(x, pad=5)


def test_greedy_decode_rules():
    C = 7
    # every frame another non-blank class: lens = T
    am = (np.arange(130) % (C - 1) + 1)[None]
    assert [len(s) for s in _decode_both(_frames(am, C))] == [130]
    # a, X, a with X >= ncharacter keeps both a: the cut-off does not reset the repeat rule, X still separates them;
    # a, a, X, X, a keeps two; a, blank, a keeps two
    am = np.array([[2, 5, 2, 0, 0, 0], [2, 2, 5, 5, 2, 6], [2, 0, 2, 2, 6, 6]])
    assert _decode_both(_frames(am, C), ncharacter=5) == [[2, 2], [2, 2], [2, 2]]
    assert _decode_both(_frames(am, C)) == [[2, 5, 2], [2, 5, 2, 6], [2, 2, 6]]
    assert _decode_both(_frames(am, C), ncharacter=1) == [[], [], []]
    # one class: nothing but the blank
    assert _decode_both(np.random.default_rng(1).standard_normal((2, 9, 1)).astype(np.float32)) == [[], []]


@pytest.mark.parametrize("T", [8192, 8193, 16384])
def test_greedy_decode_up_to_the_frame_limit(T):
    """2 * T ints of dynamic LDS: 64 KB at T = 8192, more above (the launch needs the attribute), 128 KB at the limit"""
    rng = np.random.default_rng(T)
    am = rng.integers(0, 4, size=(2, T))
    am[1, -3:] = [1, 2, 3]                       # the last frames are kept: positions near T are written
    want = _decode_both(_frames(am, 4), ncharacter=3)
    assert all(len(s) > T // 4 for s in want)


def test_greedy_decode_refuses_more_than_16384_frames_without_launching():
    lib, _, ptr, stream, _, _ = _api()
    B, T, C = 1, 16385, 4
    logits = torch.zeros(B, T, C, device="cuda")
    idx = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    assert lib.htrvt_ctc_greedy_decode(ptr(logits), B, T, C, C, C, ptr(idx), ptr(lens), stream()) != 0
    assert b"bad shape" in lib.htrvt_last_error()
    assert lib.htrvt_ctc_greedy_decode(ptr(logits), B, 16, C, C - 1, C, ptr(idx), ptr(lens), stream()) != 0      # ld < C
    torch.cuda.synchronize()
    assert (idx == -7).all() and (lens == -7).all()
