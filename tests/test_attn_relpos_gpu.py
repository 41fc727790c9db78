"""Table-driven fused attention of the window-attention fork (csrc/attn_relpos.hip: htrvt_attn_relpos_*) against a float64
restatement of the reference's Attention.forward + Block._attend (model_window/model/HTR_VT.py:33-62,113-154: zero pad to a
multiple of the window, key padding mask, roll, 1-D partition, per-window attention with the relative-position table,
reverse, unpad); its table gradient is deterministic (no atomics) and entries no pair uses get exactly zero."""
import ctypes

import pytest
import torch

from attn_refs import windowed_reference as _reference

pytestmark = pytest.mark.gpu

CASES = [(N, hd, ws, shift) for N in (64, 128, 200, 256) for hd in (64, 128) for ws, shift in ((0, 0), (16, 0), (16, 8))]


def _inputs(B, N, h, hd, P, seed):
    g = torch.Generator().manual_seed(seed)
    D = h * hd
    qkv = torch.randn(B * N, 3 * D, generator=g).to(torch.bfloat16)
    table = torch.randn(2 * P - 1, h, generator=g) * 0.5
    dout = torch.randn(B * N, D, generator=g).to(torch.bfloat16)
    return qkv, table, dout


def _run(qkv, table, dout, B, N, h, P, ws, shift):
    from htrvt_amd import variants as V
    qd = qkv.cuda().requires_grad_(True)
    td = table.cuda().requires_grad_(True)
    out = V.relpos_self_attention(qd, td, B, N, h, P, ws, shift)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    return out.detach(), qd.grad, td.grad


def _gate(name, got, want, tol=3e-2, cos_min=0.9995):
    got = got.double().cpu()
    e = (got - want).abs().max().item() / want.abs().max().item()
    cos = float((got.flatten() @ want.flatten()) / (got.norm() * want.norm()))
    print(f"   {name}: rel-to-max {e:.3e} cosine {cos:.6f}")
    assert e < tol and cos > cos_min, (name, e, cos)


@pytest.mark.parametrize("N,hd,ws,shift", CASES, ids=lambda v: str(v))
def test_relpos_attention_against_float64_reference(N, hd, ws, shift):
    from htrvt_amd import variants as V
    B, h, P = 2, 2, 320            # P > N: full attention leaves table entries unused too
    qkv, table, dout = _inputs(B, N, h, hd, P, 100 + N + hd + ws + shift)
    qr = qkv.double().clone().requires_grad_(True)
    tr = table.double().clone().requires_grad_(True)
    ref = _reference(qr, tr, B, N, h, hd, P, ws, shift)
    ref.backward(dout.double())

    out, dq, dt = _run(qkv, table, dout, B, N, h, P, ws, shift)
    err = (out.double().cpu() - ref.detach()).abs().max().item()
    print(f"N={N} hd={hd} ws={ws} shift={shift}: out max-abs {err:.3e}")
    assert err < 2.5e-2, err                                  # the bf16 gates of tests/test_variants_gpu.py
    _gate("dqkv", dq, qr.grad)
    _gate("dtable", dt, tr.grad)

    # entries of the table no (query, key) pair uses get exactly zero gradient
    idx, inside = V.relative_position_index(N, P, ws, shift)
    used = torch.zeros(2 * P - 1, dtype=torch.bool)
    used[idx[inside]] = True
    assert (~used).any()
    assert float(dt.cpu()[~used].abs().max()) == 0.0

    # bitwise reproducible: the table gradient is reduced in a fixed order, no atomics
    out2, dq2, dt2 = _run(qkv, table, dout, B, N, h, P, ws, shift)
    assert torch.equal(out, out2) and torch.equal(dq, dq2) and torch.equal(dt, dt2)


@pytest.mark.parametrize("N,ws,shift", [(128, 0, 0), (128, 16, 8), (256, 16, 0), (200, 16, 8)])
def test_relpos_agrees_with_dense_bias_route(N, ws, shift):
    """same result as the dense [heads, ld, ld] bias through the BIAS flavour of the fused kernels (padded to 128)"""
    from htrvt_amd import variants as V
    B, h, hd, P = 3, 6, 128, 256
    qkv, table, dout = _inputs(B, N, h, hd, P, 7 + N + ws)
    out, dq, dt = _run(qkv, table, dout, B, N, h, P, ws, shift)
    qd = qkv.cuda().requires_grad_(True)
    td = table.cuda().requires_grad_(True)
    bias = V.relative_position_bias(td, N, P, ws, shift, ld=V.padded_len(N, torch.bfloat16, hd))
    o2 = V.biased_self_attention(qd, bias, B, N, h)
    o2.backward(dout.cuda())
    _gate("out", out, o2.detach().double().cpu(), tol=2e-2, cos_min=0.9999)
    _gate("dqkv", dq, qd.grad.double().cpu(), tol=2e-2, cos_min=0.9999)
    _gate("dtable", dt, td.grad.double().cpu(), tol=1e-2, cos_min=0.99999)


def test_relpos_table_gradient_accumulates():
    """the C ABI adds into dtable (the rule of parameter gradients); dtable = NULL skips the table reduction"""
    from htrvt_amd import _lib
    from htrvt_amd import variants as V
    from htrvt_amd.ops import dt as dtcode, ptr, stream
    B, N, h, hd, P, ws, shift = 2, 200, 2, 64, 200, 16, 8
    qkv, table, dout = _inputs(B, N, h, hd, P, 5)
    out, dq, dt = _run(qkv, table, dout, B, N, h, P, ws, shift)
    q, t, o, d = qkv.cuda(), table.cuda(), out.contiguous(), dout.cuda()
    lse = torch.empty(B * h, N, dtype=torch.float32, device="cuda")
    o_chk = torch.empty_like(o)
    bf = dtcode(torch.bfloat16)
    _lib.check(_lib.lib.htrvt_attn_relpos_fwd(ptr(q), ptr(t), ptr(o_chk), ptr(lse), B, N, h, hd, hd ** -0.5, P, ws, shift, bf,
                                              stream()), "fwd")
    delta = torch.empty(B * h, N, dtype=torch.float32, device="cuda")
    work = torch.empty(V.relpos_workspace_floats(B, N, h, P, ws, shift), dtype=torch.float32, device="cuda")
    acc = torch.ones_like(t)
    dq2 = torch.empty_like(q)
    _lib.check(_lib.lib.htrvt_attn_relpos_bwd(ptr(q), ptr(t), ptr(o_chk), ptr(d), ptr(lse), ptr(delta), ptr(dq2), ptr(acc),
                                              ptr(work), B, N, h, hd, hd ** -0.5, P, ws, shift, bf, stream()), "bwd")
    dq3 = torch.empty_like(q)
    _lib.check(_lib.lib.htrvt_attn_relpos_bwd(ptr(q), ptr(t), ptr(o_chk), ptr(d), ptr(lse), ptr(delta), ptr(dq3), None, None,
                                              B, N, h, hd, hd ** -0.5, P, ws, shift, bf, stream()), "bwd, no dtable")
    torch.cuda.synchronize()
    assert torch.equal(o_chk, out)
    assert torch.equal(acc, 1.0 + dt)
    assert torch.equal(dq2, dq) and torch.equal(dq3, dq)


@pytest.mark.parametrize("N,hd,dtype,P,ws,shift,why", [
    (256, 128, torch.bfloat16, 128, 0, 0, "exceeds num_patches"),
    (128, 128, torch.bfloat16, 128, 16, 16, "shift=16 outside"),
    (128, 128, torch.bfloat16, 128, 16, -1, "shift=-1 outside"),
    (128, 128, torch.bfloat16, 128, 0, 4, "without a window"),
    (128, 128, torch.bfloat16, 128, -4, 0, "window=-4"),
    (48, 128, torch.bfloat16, 128, 64, 8, "at least two windows"),
    (16, 128, torch.bfloat16, 128, 0, 0, "N=16 < 32"),
    (128, 32, torch.bfloat16, 128, 0, 0, "head dim 32"),
    (128, 128, torch.float32, 128, 0, 0, "bfloat16 only"),
    (128, 128, torch.bfloat16, 4096, 0, 0, "num_patches=4096"),
])
def test_relpos_refuses_bad_geometry(N, hd, dtype, P, ws, shift, why):
    from htrvt_amd import _lib
    from htrvt_amd import variants as V
    from htrvt_amd.ops import dt as dtcode
    lib = _lib.lib
    assert lib.htrvt_attn_relpos_supported(N, hd, dtcode(dtype), P, ws, shift) == 0
    assert why in lib.htrvt_last_error().decode()
    if hd in (64, 128) and dtype == torch.bfloat16:
        assert lib.htrvt_attn_relpos_bwd_workspace_floats(2, N, 2, P, ws, shift) == -1
        assert why in lib.htrvt_last_error().decode()
    # the launches refuse before touching memory (NULL-free dummy pointers of a real buffer)
    buf = torch.zeros(1024, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    rc = lib.htrvt_attn_relpos_fwd(p, p, p, p, 2, N, 2, hd, 0.1, P, ws, shift, dtcode(dtype), None)
    assert rc != 0 and why in lib.htrvt_last_error().decode()
    rc = lib.htrvt_attn_relpos_bwd(p, p, p, p, p, p, p, p, p, 2, N, 2, hd, 0.1, P, ws, shift, dtcode(dtype), None)
    assert rc != 0 and why in lib.htrvt_last_error().decode()
    if dtype == torch.bfloat16 and hd in (64, 128):
        with pytest.raises(ValueError):
            V.relpos_self_attention(torch.zeros(2 * N, 6 * hd, dtype=dtype, device="cuda"),
                                    torch.zeros(2 * P - 1, 2, device="cuda"), 2, N, 2, P, ws, shift)


@pytest.mark.parametrize("N,ws,shift", [(128, 0, 0), (200, 16, 8)])
def test_relpos_float32_route_against_float64_reference(N, ws, shift):
    """float32 inputs take the dense-bias route of relpos_self_attention (relative_position_bias + biased_self_attention)"""
    from htrvt_amd import variants as V
    B, h, hd, P = 2, 2, 64, 256
    qkv, table, dout = _inputs(B, N, h, hd, P, 11 + N)
    qkv, dout = qkv.float(), dout.float()
    qr = qkv.double().clone().requires_grad_(True)
    tr = table.double().clone().requires_grad_(True)
    ref = _reference(qr, tr, B, N, h, hd, P, ws, shift)
    ref.backward(dout.double())
    qd = qkv.cuda().requires_grad_(True)
    td = table.cuda().requires_grad_(True)
    out = V.relpos_self_attention(qd, td, B, N, h, P, ws, shift)
    out.backward(dout.cuda())
    assert (out.detach().double().cpu() - ref.detach()).abs().max().item() < 2e-5
    _gate("dqkv", qd.grad, qr.grad, tol=1e-4, cos_min=0.999999)
    _gate("dtable", td.grad, tr.grad, tol=1e-4, cos_min=0.999999)
    with pytest.raises(TypeError):
        V.relpos_self_attention(qd.detach().bfloat16(), td.detach().bfloat16(), B, N, h, P, ws, shift)
