"""The three operators of the LGP fork's block (csrc/lgp.hip: htrvt_attn_local_*, htrvt_lgp_pool_norm_*, htrvt_lgp_upsample_*)
against float64 torch restatements of model_lgp/model/plg.py on the same (for bfloat16: bfloat16-rounded) unit-scale inputs.

Gates (those of tests/test_attn_relpos_gpu.py, the kernels these sit beside): bfloat16 forward max-abs < 2.5e-2, gradients
3e-2 of the tensor's maximum with cosine > 0.9995; float32 window attention forward max-abs < 2e-5, gradients 1e-4 of the
maximum with cosine > 0.999999.  Pooling + LayerNorm and up-sampling in float32, forward and backward, d logit_alpha
included: 1e-5 of the output's maximum (of the value, for the scalar).  These are gates on a whole tensor; the per-element
gates of the window attention kernels live in tests/test_window_edges_gpu.py (references and error model:
tests/window_refs.py, proved on the host by tests/test_window_refs_cpu.py)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from window_refs import ref_local

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
LENGTHS = (64, 100, 200, 256)


def _gate(name, got, want, tol=3e-2, cos_min=0.9995):
    got = got.double().cpu()
    e = (got - want).abs().max().item() / want.abs().max().item()
    cos = float((got.flatten() @ want.flatten()) / (got.norm() * want.norm()))
    print(f"   {name}: rel-to-max {e:.3e} cosine {cos:.7f}")
    assert e < tol and cos > cos_min, (name, e, cos)


def _grad_gate(dtype):
    return dict(tol=3e-2, cos_min=0.9995) if dtype == torch.bfloat16 else dict(tol=1e-4, cos_min=0.999999)


def _rounded(t, dtype):
    """unit-scale test data every side can hold exactly"""
    return t.to(dtype).float()


# ---------------------------------------------------------------------------------------------- window attention
_ref_local = ref_local            # WindowMHSA1D.forward restated in float64: tests/window_refs.py holds it now


def _local_inputs(B, N, h, hd, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    D = h * hd
    qkv = _rounded(torch.randn(B * N, 3 * D, generator=g), dtype)
    bias = _rounded(torch.randn(3 * D, generator=g), dtype)
    dout = _rounded(torch.randn(B * N, D, generator=g), dtype)
    return qkv, bias, dout


def _run_local(qkv, bias, dout, B, N, h, w, dtype):
    from htrvt_amd import variants as V
    qd = qkv.to(dtype).cuda().requires_grad_(True)
    bd = bias.cuda().requires_grad_(True)
    out = V.local_window_attention(qd, bd, B, N, h, w)
    out.backward(dout.to(dtype).cuda())
    torch.cuda.synchronize()
    return out.detach(), qd.grad, bd.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("N", LENGTHS)
def test_local_attention_against_float64_reference(N, hd, dtype):
    B, h, w = 3, 2, 12
    D = h * hd
    qkv, bias, dout = _local_inputs(B, N, h, hd, dtype, 300 + N + hd)
    qr = qkv.double().requires_grad_(True)
    br = bias.double().requires_grad_(True)
    ref = _ref_local(qr, br, B, N, h, hd, w)
    ref.backward(dout.double())
    assert N % w != 0 and float(br.grad[D:].abs().max()) > 0          # every length here is ragged for 12

    out, dq, db = _run_local(qkv, bias, dout, B, N, h, w, dtype)
    err = (out.double().cpu() - ref.detach()).abs().max().item()
    print(f"N={N} hd={hd} {dtype}: out max-abs {err:.3e}")
    assert err < (2.5e-2 if dtype == torch.bfloat16 else 2e-5), err
    _gate("dqkv", dq, qr.grad, **_grad_gate(dtype))
    # the padding keys' gradient, on its own: into the k and v thirds of the bias, nothing into the q third
    _gate("dbias[k, v]", db[D:], br.grad[D:], **_grad_gate(dtype))
    assert float(db[:D].abs().max()) == 0.0 and float(br.grad[:D].abs().max()) == 0.0

    out2, dq2, db2 = _run_local(qkv, bias, dout, B, N, h, w, dtype)
    assert torch.equal(out, out2) and torch.equal(dq, dq2) and torch.equal(db, db2)


def test_local_attention_masking_the_padding_would_be_wrong():
    """the trap the kernel exists for: with the padding keys masked instead, the last window moves by far more than rounding"""
    B, N, h, hd, w = 2, 200, 2, 128, 12
    qkv, bias, dout = _local_inputs(B, N, h, hd, torch.float32, 9)
    ref = _ref_local(qkv.double(), bias.double(), B, N, h, hd, w)
    out, _, _ = _run_local(qkv, bias, dout, B, N, h, w, torch.float32)
    x = qkv.double().reshape(B, N, 3, h, hd)[:, N - N % w:]
    q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
    masked = (((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, N % w, h * hd)
    last = ref.reshape(B, N, -1)[:, N - N % w:]
    assert (masked - last).abs().max().item() > 1e-2
    assert (out.double().cpu().reshape(B, N, -1)[:, N - N % w:] - last).abs().max().item() < 2e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("w", (1, 2, 3, 4, 7, 13, 16))
def test_local_attention_other_windows(w, hd, dtype):
    """every window htrvt_attn_local_supported accepts at its edges, odd ones included (the bfloat16 kernels take rows two
    at a time: an odd window's last row goes with weight 0 for its partner)"""
    from htrvt_amd import variants as V
    assert V.local_attention_supported(hd, w, dtype)
    _check_local(2, 100, 2, hd, w, dtype, 40 + w + hd)


def _check_local(B, N, h, hd, w, dtype, seed):
    qkv, bias, dout = _local_inputs(B, N, h, hd, dtype, seed)
    qr = qkv.double().requires_grad_(True)
    br = bias.double().requires_grad_(True)
    ref = _ref_local(qr, br, B, N, h, hd, w)
    ref.backward(dout.double())
    out, dq, db = _run_local(qkv, bias, dout, B, N, h, w, dtype)
    err = (out.double().cpu() - ref.detach()).abs().max().item()
    print(f"N={N} w={w} hd={hd} {dtype}: out max-abs {err:.3e}")
    assert err < (2.5e-2 if dtype == torch.bfloat16 else 2e-5), err
    _gate("dqkv", dq, qr.grad, **_grad_gate(dtype))
    if N % w:
        _gate("dbias", db[h * hd:], br.grad[h * hd:], **_grad_gate(dtype))
    else:
        assert float(db.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("hd", (64, 128))
def test_local_attention_fewer_units_than_waves(hd, dtype):
    """one image, one head, 20 tokens in windows of 12: two units, the second ragged with four padding slots, in workgroups
    of up to four waves -- the waves past the last unit must stage and write nothing"""
    _check_local(1, 20, 1, hd, 12, dtype, 77 + hd)


@pytest.mark.parametrize("N", (96, 240))
def test_local_attention_agrees_with_relpos_kernels_without_padding(N):
    """no padding (N a multiple of 12): the table-driven kernels with a zero table and window 12 compute the same thing"""
    from htrvt_amd import variants as V
    B, h, hd, w, P = 3, 6, 128, 12, 256
    qkv, bias, dout = _local_inputs(B, N, h, hd, torch.bfloat16, 70 + N)
    out, dq, db = _run_local(qkv, bias, dout, B, N, h, w, torch.bfloat16)
    assert float(db.abs().max()) == 0.0
    qd = qkv.bfloat16().cuda().requires_grad_(True)
    table = torch.zeros(2 * P - 1, h, device="cuda")
    o2 = V.relpos_self_attention(qd, table, B, N, h, P, w, 0)
    o2.backward(dout.bfloat16().cuda())
    _gate("out", out, o2.detach().double().cpu(), tol=2e-2, cos_min=0.9999)
    _gate("dqkv", dq, qd.grad.double().cpu(), tol=2e-2, cos_min=0.9999)


def test_local_attention_refusals():
    from htrvt_amd import _lib
    from htrvt_amd.ops import dt as dtcode
    lib = _lib.lib
    bf = dtcode(torch.bfloat16)
    assert lib.htrvt_attn_local_supported(128, 12, bf) == 1 and lib.htrvt_attn_local_supported(64, 12, dtcode(torch.float32)) == 1
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    for hd, w, dti, why in ((128, 0, bf, "window=0"), (128, 17, bf, "window=17"), (32, 12, bf, "head dim 32"), (128, 12, 7, "dtype 7")):
        assert lib.htrvt_attn_local_supported(hd, w, dti) == 0
        assert why in lib.htrvt_last_error().decode()
        assert lib.htrvt_attn_local_fwd(p, p, p, 1, 8, 1, hd, w, 0.1, dti, None) != 0
        assert why in lib.htrvt_last_error().decode()
        assert lib.htrvt_attn_local_bwd(p, p, p, p, p, 1, 8, 1, hd, w, 0.1, dti, None) != 0
        assert why in lib.htrvt_last_error().decode()
    assert lib.htrvt_attn_local_fwd(p, None, p, 1, 8, 1, 64, 12, 0.1, bf, None) != 0
    assert "null" in lib.htrvt_last_error().decode()
    assert lib.htrvt_attn_local_bwd(p, p, p, p, None, 1, 8, 1, 64, 12, 0.1, bf, None) != 0
    assert "null" in lib.htrvt_last_error().decode()
    assert lib.htrvt_lgp_pool_norm_fwd(p, p, p, p, 1, 8, 16, 64, 1e-5, bf, None) != 0          # G > N
    assert "G=16" in lib.htrvt_last_error().decode()
    assert lib.htrvt_lgp_pool_norm_fwd(p, None, p, p, 1, 8, 8, 64, 1e-5, bf, None) != 0
    assert "null" in lib.htrvt_last_error().decode()
    assert lib.htrvt_lgp_upsample_fwd(p, p, p, 60, 1, 8, 8, 64, bf, None) != 0                 # row stride below D
    assert "ldo=60" in lib.htrvt_last_error().decode()
    assert lib.htrvt_lgp_upsample_bwd(p, 64, p, p, p, p, None, 1, 8, 8, 64, bf, None) != 0
    assert "null" in lib.htrvt_last_error().decode()
    # 16-byte vectors throughout: a misaligned base pointer (e.g. a column offset that is no multiple of 8 bfloat16) is refused
    q = ctypes.c_void_p(buf.data_ptr() + 4)
    for rc in (lib.htrvt_attn_local_fwd(q, p, p, 1, 8, 1, 64, 12, 0.1, bf, None),
               lib.htrvt_attn_local_bwd(p, p, q, p, p, 1, 8, 1, 64, 12, 0.1, bf, None),
               lib.htrvt_lgp_pool_norm_fwd(p, q, p, p, 1, 8, 8, 64, 1e-5, bf, None),
               lib.htrvt_lgp_pool_norm_bwd(p, p, p, p, q, 1, 8, 8, 64, 0, bf, None),
               lib.htrvt_lgp_upsample_fwd(p, p, q, 64, 1, 8, 8, 64, bf, None),
               lib.htrvt_lgp_upsample_bwd(q, 64, p, p, p, p, p, 1, 8, 8, 64, bf, None)):
        assert rc != 0 and "16-byte aligned" in lib.htrvt_last_error().decode()
    with pytest.raises(ValueError):
        from htrvt_amd import variants as V
        V.local_window_attention(torch.zeros(16, 3 * 64, device="cuda"), torch.zeros(3 * 64, device="cuda"), 2, 8, 1, 17)


# ---------------------------------------------------------------------------------------------- pooling + LayerNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("N", LENGTHS)
def test_pool_norm_against_float64_reference(N, dtype):
    from htrvt_amd import variants as V
    B, D, eps = 3, 768, 1e-5
    G = min(64, N)
    g = torch.Generator().manual_seed(500 + N)
    x = _rounded(torch.randn(B * N, D, generator=g) + 0.5 * torch.randn(1, D, generator=g), dtype)
    dz = _rounded(torch.randn(B * G, D, generator=g), dtype)
    xr = x.double().requires_grad_(True)
    pooled = F.adaptive_avg_pool1d(xr.reshape(B, N, D).transpose(1, 2), G).transpose(1, 2)
    ref = F.layer_norm(pooled, (D,), eps=eps).reshape(B * G, D)
    ref.backward(dz.double())

    def run():
        xd = x.to(dtype).cuda().requires_grad_(True)
        z = V.pool_norm(xd, B, N, G, eps)
        z.backward(dz.to(dtype).cuda())
        torch.cuda.synchronize()
        return z.detach(), xd.grad

    z, dx = run()
    if dtype == torch.bfloat16:
        err = (z.double().cpu() - ref.detach()).abs().max().item()
        print(f"N={N}: z max-abs {err:.3e}")
        assert err < 2.5e-2, err
    else:
        _gate("z", z, ref.detach(), tol=1e-5, cos_min=0.999999)
    _gate("dx", dx, xr.grad, **(_grad_gate(dtype) if dtype == torch.bfloat16 else dict(tol=1e-5, cos_min=0.999999)))
    z2, dx2 = run()
    assert torch.equal(z, z2) and torch.equal(dx, dx2)


def test_pool_norm_backward_accumulates():
    from htrvt_amd import _lib
    from htrvt_amd.ops import dt as dtcode, ptr, stream
    B, N, G, D = 2, 200, 64, 256
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * N, D, generator=g).cuda()
    dz = torch.randn(B * G, D, generator=g).cuda()
    z, mean, rstd = torch.empty(B * G, D, device="cuda"), torch.empty(B * G, device="cuda"), torch.empty(B * G, device="cuda")
    f32 = dtcode(torch.float32)
    lib = _lib.lib
    _lib.check(lib.htrvt_lgp_pool_norm_fwd(ptr(x), ptr(z), ptr(mean), ptr(rstd), B, N, G, D, 1e-5, f32, stream()))
    pooled = F.adaptive_avg_pool1d(x.cpu().double().reshape(B, N, D).transpose(1, 2), G).transpose(1, 2).reshape(B * G, D)
    assert (mean.cpu().double() - pooled.mean(-1)).abs().max().item() < 1e-6
    assert ((rstd.cpu().double() - (pooled.var(-1, unbiased=False) + 1e-5).rsqrt()).abs() / rstd.cpu().double()).max().item() < 1e-5
    ws = torch.empty(2 * B * G, device="cuda")
    d0 = torch.empty(B * N, D, device="cuda")
    base = torch.randn(B * N, D, generator=g).cuda()
    d1 = base.clone()
    _lib.check(lib.htrvt_lgp_pool_norm_bwd(ptr(dz), ptr(z), ptr(rstd), ptr(ws), ptr(d0), B, N, G, D, 0, f32, stream()))
    _lib.check(lib.htrvt_lgp_pool_norm_bwd(ptr(dz), ptr(z), ptr(rstd), ptr(ws), ptr(d1), B, N, G, D, 1, f32, stream()))
    torch.cuda.synchronize()
    assert torch.equal(d1, base + d0)


# ---------------------------------------------------------------------------------------------- up-sampling
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("N", LENGTHS)
def test_upsample_against_float64_reference(N, dtype):
    from htrvt_amd import variants as V
    B, D = 3, 768
    G = min(64, N)
    g = torch.Generator().manual_seed(700 + N)
    y = _rounded(torch.randn(B * G, D, generator=g), dtype)
    dout = _rounded(torch.randn(B * N, D, generator=g), dtype)
    alpha = torch.tensor(-0.37)
    yr = y.double().requires_grad_(True)
    ar = alpha.double().requires_grad_(True)
    up = F.interpolate(yr.reshape(B, G, D).transpose(1, 2), size=N, mode="linear", align_corners=False).transpose(1, 2)
    ref = (up * torch.sigmoid(ar)).reshape(B * N, D)
    ref.backward(dout.double())

    def run():
        yd = y.to(dtype).cuda().requires_grad_(True)
        ad = alpha.cuda().requires_grad_(True)
        out = V.upsample_scale(yd, ad, B, G, N)
        out.backward(dout.to(dtype).cuda())
        torch.cuda.synchronize()
        return out.detach(), yd.grad, ad.grad

    out, dy, da = run()
    assert da.shape == alpha.shape
    rel = abs(da.item() - ar.grad.item()) / abs(ar.grad.item())
    print(f"N={N} {dtype}: dalpha {da.item():.6f} ref {ar.grad.item():.6f} rel {rel:.3e}")
    if dtype == torch.bfloat16:
        err = (out.double().cpu() - ref.detach()).abs().max().item()
        assert err < 2.5e-2, err
        _gate("dy", dy, yr.grad)
        assert rel < 3e-2
    else:
        _gate("out", out, ref.detach(), tol=1e-5, cos_min=0.999999)
        _gate("dy", dy, yr.grad, tol=1e-5, cos_min=0.999999)
        assert rel < 1e-5, rel
    out2, dy2, da2 = run()
    assert torch.equal(out, out2) and torch.equal(dy, dy2) and torch.equal(da, da2)


def test_upsample_strided_rows_and_accumulating_alpha_gradient():
    """the forward writes the right half of a [B N][2D] operand in place, the backward reads its gradient from there;
    d logit_alpha is a parameter gradient and accumulates"""
    from htrvt_amd import _lib
    from htrvt_amd.ops import dt as dtcode, ptr, stream
    B, N, G, D = 2, 200, 64, 256
    g = torch.Generator().manual_seed(4)
    bf = dtcode(torch.bfloat16)
    lib = _lib.lib
    y = torch.randn(B * G, D, generator=g).bfloat16().cuda()
    alpha = torch.tensor(0.2).cuda()
    dense = torch.empty(B * N, D, dtype=torch.bfloat16, device="cuda")
    wide = torch.full((B * N, 2 * D), 7.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.htrvt_lgp_upsample_fwd(ptr(y), ptr(alpha), ptr(dense), D, B, N, G, D, bf, stream()))
    _lib.check(lib.htrvt_lgp_upsample_fwd(ptr(y), ptr(alpha), wide.data_ptr() + 2 * D, 2 * D, B, N, G, D, bf, stream()))
    torch.cuda.synchronize()
    assert torch.equal(wide[:, D:], dense) and bool((wide[:, :D] == 7.0).all())
    dwide = torch.randn(B * N, 2 * D, generator=g).bfloat16().cuda()
    ddense = dwide[:, D:].contiguous()
    nws = lib.htrvt_lgp_upsample_bwd_workspace_floats(B, G)
    ws = torch.empty(nws, device="cuda")
    dy0, dy1 = torch.empty_like(y), torch.empty_like(y)
    da0, da1 = torch.zeros((), device="cuda"), torch.full((), 1.5, device="cuda")
    _lib.check(lib.htrvt_lgp_upsample_bwd(ptr(ddense), D, ptr(y), ptr(alpha), ptr(dy0), ptr(da0), ptr(ws), B, N, G, D, bf, stream()))
    _lib.check(lib.htrvt_lgp_upsample_bwd(dwide.data_ptr() + 2 * D, 2 * D, ptr(y), ptr(alpha), ptr(dy1), ptr(da1), ptr(ws), B, N, G,
                                          D, bf, stream()))
    torch.cuda.synchronize()
    assert torch.equal(dy0, dy1)
    assert da1.item() == (torch.full((), 1.5, device="cuda") + da0).item()
