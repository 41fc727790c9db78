"""The shifted local-window attention kernels (csrc/lgp.hip: htrvt_attn_local_shift_*) against a float64 torch restatement
of WindowMHSA1D.forward of the SGM local-global fork (model_sgm_localglobal/model/HTR_VT.py:118-152) applied to the qkv
Linear's output: roll by `shift`, pad with rows equal to the bias (what the Linear makes of a zero token), attend inside the
windows, crop, roll back.  Same (for bfloat16: bfloat16-rounded) unit-scale inputs on both sides.

Gates: `_gate` / `_grad_gate` of tests/test_lgp_kernels_gpu.py, the unshifted kernel's (float32 1e-4 of the maximum with
cosine > 0.999999, bfloat16 3e-2 with cosine > 0.9995), and its forward max-abs bounds (2e-5 / 2.5e-2).  The per-element
gates of these kernels (wrap and padding rows in one window, every window size) live in tests/test_window_edges_gpu.py."""
import ctypes

import pytest
import torch

from test_lgp_kernels_gpu import DTYPES, _gate, _grad_gate, _local_inputs
from window_refs import ref_shifted

pytestmark = pytest.mark.gpu

B, HEADS = 2, 2


_ref_shifted = ref_shifted        # the shifted WindowMHSA1D.forward restated in float64: tests/window_refs.py holds it now


def _run(qkv, bias, dout, N, h, w, s, dtype):
    from htrvt_amd import variants as V
    qd = qkv.to(dtype).cuda().requires_grad_(True)
    bd = bias.cuda().requires_grad_(True)
    out = V.local_window_attention(qd, bd, B, N, h, w, s)
    out.backward(dout.to(dtype).cuda())
    torch.cuda.synchronize()
    return out.detach(), qd.grad, bd.grad


def _check(N, hd, w, s, dtype, seed):
    D = HEADS * hd
    qkv, bias, dout = _local_inputs(B, N, HEADS, hd, dtype, seed)
    assert float(bias.abs().min()) > 0
    qr = qkv.double().requires_grad_(True)
    br = bias.double().requires_grad_(True)
    ref = _ref_shifted(qr, br, B, N, HEADS, hd, w, s)
    ref.backward(dout.double())
    out, dq, db = _run(qkv, bias, dout, N, HEADS, w, s, dtype)
    err = (out.double().cpu() - ref.detach()).abs().max().item()
    print(f"N={N} w={w} shift={s} hd={hd} {dtype}: out max-abs {err:.3e}")
    assert err < (2.5e-2 if dtype == torch.bfloat16 else 2e-5), err
    _gate("out", out, ref.detach(), **_grad_gate(dtype))
    _gate("dqkv", dq, qr.grad, **_grad_gate(dtype))
    assert float(db[:D].abs().max()) == 0.0                 # nothing into the q third
    if N % w:        # dpad: the padding keys' gradient, summed over the images into the k and v thirds of the bias
        assert float(br.grad[:D].abs().max()) == 0.0 and float(br.grad[D:].abs().max()) > 0
        _gate("dbias[k, v]", db[D:], br.grad[D:], **_grad_gate(dtype))
    else:            # no padding key: the reference's bias takes no part, the kernel's dpad is cleared
        assert br.grad is None and float(db.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("N", (8, 12, 64, 128, 200))
def test_shifted_local_attention_against_float64_reference(N, hd, dtype):
    """N = 8: shorter than a window (shift 11 rolls by 11 mod 8); 12: exactly one window, no padding; 64: pad 8; 128: pad 4;
    200: pad 4 and, shifted, a ragged window (tokens 200 - s - 8 ... 200 - s - 1) that is not the wrap window"""
    for s in (0, 6, 11):
        _check(N, hd, 12, s, dtype, 900 + N + hd + s)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_shifted_local_attention_window_16(dtype):
    _check(40, 128, 16, 8, dtype, 77)
    _check(40, 64, 16, 8, dtype, 78)


def _raw(fn_fwd, fn_bwd, qkv, bias, dout, N, h, hd, w, extra):
    from htrvt_amd.ops import dt, ptr, stream
    D = h * hd
    out = torch.full((B * N, D), 3.0, dtype=qkv.dtype, device="cuda")
    dqkv = torch.full_like(qkv, 3.0)
    dpad = torch.full((B, 2 * D), 3.0, dtype=torch.float32, device="cuda")
    sc, dti = hd ** -0.5, dt(qkv.dtype)
    assert fn_fwd(ptr(qkv), ptr(bias), ptr(out), B, N, h, hd, w, *extra, sc, dti, stream()) == 0
    assert fn_bwd(ptr(qkv), ptr(bias), ptr(dout), ptr(dqkv), ptr(dpad), B, N, h, hd, w, *extra, sc, dti, stream()) == 0
    torch.cuda.synchronize()
    return out, dqkv, dpad


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("hd", (64, 128))
def test_shift_zero_is_bitwise_the_unshifted_entry_point(hd, dtype):
    from htrvt_amd._lib import lib
    for N in (12, 64, 200):
        qkv, bias, dout = _local_inputs(B, N, HEADS, hd, dtype, 5 + N)
        qd, bd, gd = qkv.to(dtype).cuda(), bias.cuda(), dout.to(dtype).cuda()
        old = _raw(lib.htrvt_attn_local_fwd, lib.htrvt_attn_local_bwd, qd, bd, gd, N, HEADS, hd, 12, ())
        new = _raw(lib.htrvt_attn_local_shift_fwd, lib.htrvt_attn_local_shift_bwd, qd, bd, gd, N, HEADS, hd, 12, (0,))
        for name, a, b in zip(("out", "dqkv", "dpad"), old, new):
            assert torch.equal(a, b), (N, name)
        # the shifted call is reproducible too, and does move the result (N = 12 is one window whatever the shift: the same
        # keys in another order)
        s1 = _raw(lib.htrvt_attn_local_shift_fwd, lib.htrvt_attn_local_shift_bwd, qd, bd, gd, N, HEADS, hd, 12, (6,))
        s2 = _raw(lib.htrvt_attn_local_shift_fwd, lib.htrvt_attn_local_shift_bwd, qd, bd, gd, N, HEADS, hd, 12, (6,))
        assert all(torch.equal(a, b) for a, b in zip(s1, s2))
        assert N == 12 or not torch.equal(s1[0], new[0])


def test_masking_the_wrap_would_be_wrong():
    """window 0 of the shifted block mixes the last 6 tokens of the line with its first 6 and the fork has no mask there:
    a reference that masks attention between the two groups is far (100 x the float32 gate and more) from the kernel on
    exactly those twelve tokens, the unmasked one is within the gate"""
    N, hd, w, s = 64, 128, 12, 6
    qkv, bias, dout = _local_inputs(B, N, HEADS, hd, torch.float32, 31)
    ref = _ref_shifted(qkv.double(), bias.double(), B, N, HEADS, hd, w, s)
    masked = _ref_shifted(qkv.double(), bias.double(), B, N, HEADS, hd, w, s, mask_wrap=True)
    out, _, _ = _run(qkv, bias, dout, N, HEADS, w, s, torch.float32)
    out = out.double().cpu()
    _gate("out vs unmasked", out, ref, **_grad_gate(torch.float32))
    wrap = torch.zeros(N, dtype=torch.bool)
    wrap[:w - s] = wrap[N - s:] = True
    o3, m3, r3 = (t.reshape(B, N, -1) for t in (out, masked, ref))
    assert torch.equal(m3[:, ~wrap], r3[:, ~wrap])              # the mask touches the wrap window only
    e = (o3[:, wrap] - m3[:, wrap]).abs().max().item() / ref.abs().max().item()
    print(f"masked-wrap reference vs kernel on the wrap window: rel-to-max {e:.3e} (gate 1e-4)")
    assert e > 1e-2, e


def test_shift_refusals():
    from htrvt_amd import _lib, variants as V
    from htrvt_amd.ops import dt as dtcode
    lib = _lib.lib
    bf = dtcode(torch.bfloat16)
    buf = torch.zeros(8192, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.htrvt_attn_local_shift_supported(128, 12, 6, bf) == 1 and lib.htrvt_attn_local_shift_supported(64, 12, 11, 0) == 1
    for w, s in ((12, 12), (12, -1), (16, 16), (1, 1)):
        assert lib.htrvt_attn_local_shift_supported(64, w, s, bf) == 0
        assert f"shift={s}" in lib.htrvt_last_error().decode()
        assert lib.htrvt_attn_local_shift_fwd(p, p, p, 1, 8, 1, 64, w, s, 0.1, bf, None) != 0
        assert f"shift={s}" in lib.htrvt_last_error().decode()
        assert lib.htrvt_attn_local_shift_bwd(p, p, p, p, p, 1, 8, 1, 64, w, s, 0.1, bf, None) != 0
        assert f"shift={s}" in lib.htrvt_last_error().decode()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                            # nothing was launched
    assert lib.htrvt_attn_local_shift_supported(64, 17, 0, bf) == 0 and "window=17" in lib.htrvt_last_error().decode()
    assert lib.htrvt_attn_local_shift_fwd(p, None, p, 1, 8, 1, 64, 12, 6, 0.1, bf, None) != 0
    assert "null" in lib.htrvt_last_error().decode()
    with pytest.raises(ValueError, match="shift=12"):
        V.local_window_attention(torch.zeros(16, 3 * 64, device="cuda"), torch.zeros(3 * 64, device="cuda"), 2, 8, 1, 12, 12)
