"""The references of tests/test_ctc_gpu.py on their own, without a device: the case list reaches the paths it is meant
to reach, the float64 oracle agrees with the closed form and with ATen's float64 CTC on every case, ATen's float32 CTC is
inside the bounds the kernels are held to (so a bound that a kernel misses is the kernel's doing), and the mistakes a
kernel with K states per lane can make move nll on the boundary / single-alignment cases by more than the nll bound."""
import numpy as np
import pytest
import torch

import ctc_cases as CC

NAMES = list(CC.CASES)
SINGLE = [n for n in NAMES if n.startswith("single_")]
EDGE = [n for n in NAMES if n.startswith("edge_")]


@pytest.fixture(scope="module")
def ref():
    return CC.reference


def test_case_list_reaches_every_dispatch_path():
    ks = {n: CC.lane_states(c) for n, c in CC.CASES.items()}
    assert [ks[f"edge_L{L}_T{L + 13}"] for L in (31, 32, 63, 64, 95, 96, 127)] == [1, 2, 2, 3, 3, 4, 4]
    assert [ks[f"bound_{m}"] for m in CC.BOUNDS] == [1, 3, 4, 0]
    assert [ks[f"single_L{L}"] for L in (1, 5, 32, 64, 127, 130)] == [1, 1, 2, 3, 4, 0]
    assert ks["classes_C300"] == 0 and ks["long_S521"] == 0 and ks["peaked_long"] == 0 and ks["peaked_fast"] == 2
    for k, name in CC.one_per_k().items():
        assert ks[name] == (k if isinstance(k, int) else 0) and 0 in CC.CASES[name].lengths.tolist()
    for c in CC.CASES.values():
        assert CC.cost(c) <= 250_000 and c.logits.dtype == np.float32 and c.targets.dtype == np.int32
        assert c.targets.size == c.lengths.sum() and (c.targets >= 1).all() and (c.targets < c.logits.shape[2]).all()
        assert CC.bound_of(c) >= c.lengths.max()
    # ctc_kernel: three states per thread; a label more than four times in a sample of S <= 256 states (the `rest` walk)
    assert 2 * CC.CASES["long_S521"].lengths.max() + 1 > 512
    short = CC.split(CC.CASES["long_three_labels"].targets, CC.CASES["long_three_labels"].lengths)[1]
    assert 2 * len(short) + 1 <= 256 and np.bincount(short).max() > 4
    c = CC.CASES["long_infeasible"]
    assert all(len(l) + CC.repeats(l) > c.logits.shape[1] for l in CC.split(c.targets, c.lengths))


@pytest.mark.parametrize("name", SINGLE)
def test_oracle_equals_the_closed_form_on_single_alignments(ref, name):
    c = CC.CASES[name]
    nll, grad = ref(name)
    want_nll, want_grad = CC.closed_form(c)
    assert (want_nll[0] > 0) and np.abs(nll - want_nll).max() <= 1e-12 * np.abs(want_nll).max()
    assert np.abs(grad - want_grad).max() <= 1e-12 * np.abs(want_grad).max()
    labs = CC.split(c.targets, c.lengths)
    for b, lab in enumerate(labs):
        if len(lab) + CC.repeats(lab) > c.logits.shape[1]:         # T = L + r - 1
            assert nll[b] == 0.0 and not grad[b].any()
    assert len(labs[0]) < 5 or any(nll == 0.0)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_aten_float64_and_aten_float32_is_inside_the_bounds(ref, name):
    """float64: T steps of log-sum-exp over |alpha| <= |nll| leave about T * eps64 * |nll| < 1e-10 absolute in nll and
    the same, relative, in an occupancy.  float32: the kernels' bounds must hold for a plain float32 evaluation of
    the same recursion; a case where they do not tests the number format, not the kernel"""
    c = CC.CASES[name]
    nll, grad = ref(name)
    n64, g64 = CC.aten_ctc(c, torch.float64)
    assert np.isfinite(nll).all() and np.isfinite(grad).all()
    assert np.abs(n64 - nll).max() <= 1e-12 * max(1.0, np.abs(nll).max())
    assert np.abs(g64 - grad).max() <= 1e-9 * max(np.abs(grad).max(), 1e-300)
    assert np.array_equal(n64 == 0, nll == 0)
    n32, g32 = CC.aten_ctc(c, torch.float32)
    e_n, e_g = CC.errors(n32, g32, nll, grad)
    print(f"\n{name}: ATen float32 nll error {e_n:.3f} of its bound, gradient error {e_g:.3f} of its bound")
    assert e_n <= 1.0 and e_g < 1.0


def test_every_mutant_is_caught_by_the_nll_bound(ref):
    """each mistake, applied to the longest sample of a boundary / single-alignment case, against that case's nll bound:
    every mutant is caught by at least two cases and under every K, the unmutated recursion by none"""
    caught = {m: [] for m in CC.MUTANTS}
    print()
    for name in EDGE + SINGLE:
        c = CC.CASES[name]
        nll, _ = ref(name)
        bound = CC.NLL_RTOL * max(1.0, np.abs(nll).max())
        lab = CC.split(c.targets, c.lengths)[0]
        K = CC.lane_states(c) or 4
        assert abs(CC.sample_nll(c.logits[0], lab) - nll[0]) <= 1e-12 * max(1.0, nll[0])
        row = []
        for m in CC.MUTANTS:
            d = abs(CC.sample_nll(c.logits[0], lab, m, K) - nll[0])
            row.append(f"{m} {d / bound:9.3g}")
            if d > bound:
                caught[m].append(name)
        print(f"{name:18s} K={K} nll {nll[0]:8.2f}  moved by (in bounds): " + "  ".join(row))
    for m, names in caught.items():          # never one shape per mutant, and every K instance has a case that sees it
        assert len(names) >= 2, (m, names)
        assert {CC.lane_states(CC.CASES[n]) for n in names} >= {1, 2, 3, 4}, (m, names)
    # the issue's own figures: the skip mutants at the tight and the loose T, the last state at the K = 4 edge
    assert "edge_L127_T140" in caught["skip_lost_at_lane_edge"] and "edge_L127_T256" in caught["skip_lost_at_lane_edge"]
    assert "edge_L127_T140" in caught["last_state_dropped"] and "edge_L127_T256" in caught["last_state_dropped"]
