"""Attention dropout / residual dropout, what can be checked without a device: the new C ABI is declared and exported, the
host-side argument checks answer before any launch, and the numpy restatement of the mask (tests/attn_dropout_refs.py) is
deterministic and keeps the share it should."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import attn_dropout_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["htrvt_attn_dropout_supported", "htrvt_attn_dropout_fwd", "htrvt_attn_dropout_bwd",
               "htrvt_attn_relpos_dropout_fwd", "htrvt_attn_relpos_dropout_bwd", "htrvt_residual_dropout"]
BF16, F32 = 1, 0


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import _lib
    return _lib


def test_new_symbols_are_declared_and_exported():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in L.PROTOTYPES, sym
        assert ctypes.cast(getattr(raw, sym), ctypes.c_void_p).value, sym


def test_supported_predicate():
    lib = _lib().lib
    assert lib.htrvt_attn_dropout_supported(256, 128, BF16) == 1
    assert lib.htrvt_attn_dropout_supported(256, 128, F32) == 0
    assert lib.htrvt_attn_dropout_supported(72, 32, BF16) == 1 and lib.htrvt_attn_dropout_supported(160, 64, BF16) == 1
    assert lib.htrvt_attn_dropout_supported(16, 64, BF16) == 0 and lib.htrvt_attn_dropout_supported(256, 96, BF16) == 0


@pytest.mark.parametrize("p", [1.0, -0.25])
def test_probability_outside_the_range_is_refused_before_any_launch(p):
    """null operands throughout: the probability check comes first and nothing is launched"""
    lib = _lib().lib
    calls = {
        "attn_dropout_fwd": lambda: lib.htrvt_attn_dropout_fwd(None, None, None, 1, 64, 2, 64, 0.125, None, p, BF16, None),
        "attn_dropout_bwd": lambda: lib.htrvt_attn_dropout_bwd(None, None, None, None, None, None, 1, 64, 2, 64, 0.125, None, p,
                                                               BF16, None),
        "attn_relpos_fwd": lambda: lib.htrvt_attn_relpos_dropout_fwd(None, None, None, None, 1, 64, 2, 64, 0.125, 64, 0, 0, None,
                                                                     p, BF16, None),
        "attn_relpos_bwd": lambda: lib.htrvt_attn_relpos_dropout_bwd(None, None, None, None, None, None, None, None, None, 1, 64,
                                                                     2, 64, 0.125, 64, 0, 0, None, p, BF16, None),
        "residual_dropout": lambda: lib.htrvt_residual_dropout(None, None, None, 4, 64, 8, None, p, 0.0, F32, None),
        "residual_dropout path": lambda: lib.htrvt_residual_dropout(None, None, None, 4, 64, 8, None, 0.0, p, F32, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.htrvt_last_error().decode()
        assert name.split()[0] in msg and "outside [0, 1)" in msg, (name, msg)


def test_thresholds_and_scale():
    assert R.thr_of(0.0) == 0 and R.thr_of(0.5) == 1 << 23 and R.thr_of(0.05) == 838861
    assert R.scale_of(0.5) == 2.0 and abs(R.scale_of(0.05) - 1 / 0.95) < 1e-7


def test_restated_mask_is_deterministic_and_a_function_of_the_index():
    a = R.keep_mask(1234567, 2, 3, 40, 0.5)
    assert a.dtype == np.bool_ and a.shape == (2, 3, 40, 40)
    assert np.array_equal(a, R.keep_mask(1234567, 2, 3, 40, 0.5))
    assert not np.array_equal(a, R.keep_mask(1234568, 2, 3, 40, 0.5))
    # element ((b h + head) N + q) N + k, whatever array it is asked through
    b, hh, q, k = 1, 2, 17, 5
    i = ((b * 3 + hh) * 40 + q) * 40 + k
    assert bool(R.keep_elems(1234567, [i], 0.5)[0]) == bool(a[b, hh, q, k])
    assert R.keep_mask(99, 1, 1, 32, 0.0).all()                       # p = 0 keeps everything
    # a smaller p keeps a superset (one 24-bit draw per element against a lower threshold)
    assert (R.keep_mask(5, 1, 2, 48, 0.05) | ~R.keep_mask(5, 1, 2, 48, 0.5)).all()
    # one known value of the splitmix64 finaliser: its first output from state 0 is mix64(G)
    assert int(R.mix64(np.array([R.G]))[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("p", [0.05, 0.5])
def test_restated_mask_keeps_its_share(p):
    n = 2 * 3 * 160 * 160
    share = float(R.keep_mask(2024, 2, 3, 160, p).mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"\nkeep share {share:.5f} at p={p}: {abs(share - (1 - p)) / sigma:.2f} sigma")
    assert abs(share - (1 - p)) <= 5 * sigma
