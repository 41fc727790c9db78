"""tests/kernel_refs.py against torch where torch has the operation: the closed-form BatchNorm / LayerNorm / softmax /
whiten backward against float64 autograd, the explicit arg-max scan against ATen's max_pool2d on data WITH ties, the
conv1 pieces against F.conv2d autograd.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R

F64 = torch.float64


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("rows,D", [(1, 8), (37, 1000)])
def test_layernorm_reference_matches_autograd(rows, D):
    g = torch.Generator().manual_seed(rows + D)
    x = (torch.randn(rows, D, generator=g, dtype=F64) * 0.1 + 100.0).requires_grad_(True)
    gamma = torch.randn(D, generator=g, dtype=F64).requires_grad_(True)
    beta = torch.randn(D, generator=g, dtype=F64).requires_grad_(True)
    dy, dres = torch.randn(rows, D, generator=g, dtype=F64), torch.randn(rows, D, generator=g, dtype=F64)
    y = F.layer_norm(x, (D,), gamma, beta, 1e-6)
    (y * dy).sum().backward()
    yr, mean, rstd = R.layernorm_fwd(x.detach(), gamma.detach(), beta.detach(), 1e-6)
    assert _close(yr, y.detach())
    dx, dgamma, dbeta = R.layernorm_bwd(dy, x.detach(), mean, rstd, gamma.detach(), dres)
    assert _close(dx, x.grad + dres, 1e-9) and _close(dgamma, gamma.grad, 1e-9) and _close(dbeta, beta.grad)


def test_softmax_reference_matches_autograd_and_takes_the_bias_row_modulo():
    g = torch.Generator().manual_seed(3)
    rows, n, brows = 11, 132, 4
    s = (torch.randn(rows, n, generator=g, dtype=F64) * 10).requires_grad_(True)
    bias = torch.randn(brows, n, generator=g, dtype=F64)
    bias[1, 5:] = -1e30
    bias[2, :] = -1e30                                   # a fully masked row: uniform probabilities, no NaN
    dp = torch.randn(rows, n, generator=g, dtype=F64)
    full = torch.stack([bias[r % brows] for r in range(rows)])
    p = torch.softmax(s + full, -1)
    (p * dp).sum().backward()
    pr = R.softmax_rows(s.detach(), bias)
    assert _close(pr, p.detach()) and torch.isfinite(pr).all()
    assert torch.equal(pr[2], torch.full((n,), 1.0 / n, dtype=F64)) and float(pr[1, 5:].abs().max()) == 0.0
    assert _close(R.softmax_bwd_rows(pr, dp, 0.25), 0.25 * s.grad, 1e-10)


def test_seq_whiten_reference_matches_autograd():
    g = torch.Generator().manual_seed(4)
    B, N, C = 3, 7, 9
    x = torch.randn(B, N * C, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(B, N * C, generator=g, dtype=F64)
    y = F.layer_norm(x, (N * C,), None, None, 1e-5)
    (y * dy).sum().backward()
    yr, stats = R.seq_whiten_fwd(x.detach(), 1e-5)
    assert _close(yr, y.detach()) and _close(R.seq_whiten_bwd(dy, yr, stats), x.grad, 1e-10)


@pytest.mark.parametrize("npix,C", [(37, 8), (1000, 24)])
def test_batchnorm_references_agree_with_each_other_and_with_torch(npix, C):
    g = torch.Generator().manual_seed(npix)
    x = torch.randn(npix, C, generator=g, dtype=F64) * 2 + 3
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    dy = torch.randn(npix, C, generator=g, dtype=F64)
    eps, mom = 1e-5, 0.1
    # statistics from partial sums == nn.BatchNorm's train-mode step, running statistics included
    rows = 5
    chunks = torch.tensor_split(x, rows)
    partial = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in chunks])
    rm0, rv0 = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    scale, shift, mean, rstd, rm, rv = R.bn_finalize(partial, float(npix), gamma, beta, eps, mom, rm0, rv0)
    rm_t, rv_t = rm0.clone(), rv0.clone()
    y_t = F.batch_norm(x.t()[None], rm_t, rv_t, gamma, beta, True, mom, eps)[0].t()
    assert _close(R.bn_apply(x, scale, shift), y_t, 1e-9) and _close(rm, rm_t) and _close(rv, rv_t, 1e-9)
    # eval coefficients == eval-mode batch_norm
    es, eh, er = R.bn_eval_coeffs(gamma, beta, rm, rv, eps)
    assert _close(R.bn_apply(x, es, eh), F.batch_norm(x.t()[None], rm, rv, gamma, beta, False, mom, eps)[0].t(), 1e-10)
    assert _close(er, 1.0 / torch.sqrt(rv + eps))
    # closed-form backward == autograd, == the [3][C] coefficient form
    dx_a, dg_a, db_a, mean_a, rstd_a = R.bn_bwd_autograd(dy, x, gamma, beta, eps)
    assert _close(mean, mean_a, 1e-10) and _close(rstd, rstd_a, 1e-9)
    dx, dgamma, dbeta, gm = R.bn_bwd(dy, None, x, mean_a, rstd_a, gamma, float(npix))
    assert _close(dx, dx_a, 1e-9) and _close(dgamma, dg_a, 1e-9) and _close(dbeta, db_a, 1e-9)
    _, s1, s2 = R.bn_bwd_sums(dy, None, x, mean_a, rstd_a)
    coef = R.bn_bwd_coef(s1, s2, float(npix), gamma, mean_a, rstd_a)
    assert _close(coef[0] * dy + coef[1] * x + coef[2], dx_a, 1e-9)
    # with the ReLU mask: autograd through relu(bn(x))
    xr = x.clone().requires_grad_(True)
    yact = torch.relu(F.batch_norm(xr.t()[None], None, None, gamma, beta, True, 0.0, eps)[0].t())
    (yact * dy).sum().backward()
    dx_m, _, _, g_m = R.bn_bwd(dy, yact.detach(), x, mean_a, rstd_a, gamma, float(npix))
    assert _close(dx_m, xr.grad, 1e-9) and torch.equal(g_m, dy * (yact.detach() > 0))
    # eval mode: statistics are constants
    xe = x.clone().requires_grad_(True)
    (F.batch_norm(xe.t()[None], rm, rv, gamma, beta, False, mom, eps)[0].t() * dy).sum().backward()
    dx_e, _, _, _ = R.bn_bwd(dy, None, x, rm, er, gamma, -1.0)
    ce = R.bn_bwd_coef(s1, s2, -1.0, gamma, rm, er)
    assert _close(dx_e, xe.grad, 1e-10) and _close(ce[0] * dy, xe.grad, 1e-10) and not ce[1:].any()


def test_bn_finalize_reference_count_one_keeps_the_biased_variance():
    C = 8
    partial = torch.arange(1, C + 1, dtype=F64).view(1, 1, C).repeat(1, 2, 1)
    partial[0, 1] = partial[0, 0] ** 2
    one, zero = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
    _, _, mean, rstd, rm, rv = R.bn_finalize(partial, 1.0, one, zero, 1e-5, 0.1, zero, one)
    assert torch.equal(mean, partial[0, 0]) and _close(rstd, torch.full((C,), 1e-5, dtype=F64) ** -0.5)
    assert torch.isfinite(rv).all() and _close(rv, 0.9 * one)


def test_aten_returns_the_first_maximum_of_a_tied_window():
    """the rule the header promises: for a block of equal values ATen's CPU max_pool2d returns, per window, the first
    cell in (row, column) scan order -- float32 and bfloat16 alike"""
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.ones(1, 1, 3, 3, dtype=dtype)
        _, ind = F.max_pool2d(x, 3, stride=(2, 1), padding=1, return_indices=True)
        assert ind.flatten().tolist() == [0, 0, 1, 3, 3, 4]


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 37), (32, 5), (6, 4)])
@pytest.mark.parametrize("with_bn", [False, True])
def test_argmax_scan_matches_aten_on_tied_data(H, W, with_bn):
    """values on a coarse grid (-2 .. 2): nearly every window ties.  The bytes of the explicit scan must name the same
    input element as ATen's flat index, the backward must equal autograd"""
    B, C = 2, 4
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randint(-2, 3, (B, H, W, C), generator=g).to(F64)
    scale = torch.tensor([1.0, -1.0, 0.5, 2.0], dtype=F64) if with_bn else None
    shift = torch.tensor([0.0, 1.0, -0.5, -3.0], dtype=F64) if with_bn else None
    y, idx = R.bn_relu_maxpool(x, scale, shift)
    v = (x if scale is None else torch.relu(x * scale + shift)).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y_t, ind = F.max_pool2d(v, 3, stride=(2, 1), padding=1, return_indices=True)
    assert torch.equal(y, y_t.detach().permute(0, 2, 3, 1))
    Ho = R.pooled_rows(H)
    ho = torch.arange(Ho).view(1, Ho, 1, 1)
    wo = torch.arange(W).view(1, 1, W, 1)
    open_ = idx != 15
    pos = torch.where(open_, idx, torch.zeros_like(idx)).long()
    flat = (2 * ho - 1 + pos // 3) * W + (wo - 1 + pos % 3)
    ind_nhwc = ind.permute(0, 2, 3, 1)
    assert torch.equal(flat[open_], ind_nhwc[open_])
    if with_bn:
        assert torch.equal(~open_, ~(y > 0)) and (~open_).any()
    else:
        assert open_.all()
    assert (torch.bincount(idx.flatten().long(), minlength=16)[:9] > 0).sum() >= (4 if H * W > 4 else 1)
    # backward: autograd through relu(bn(x)) -> max_pool2d
    dpool = torch.randint(-8, 9, (B, Ho, W, C), generator=g).to(F64)
    xr = x.clone().requires_grad_(True)
    vr = xr if scale is None else torch.relu(xr * scale + shift)
    (F.max_pool2d(vr.permute(0, 3, 1, 2), 3, stride=(2, 1), padding=1).permute(0, 2, 3, 1) * dpool).sum().backward()
    want = xr.grad if scale is None else xr.grad / scale          # kernels return d(bn output), not d(x)
    assert torch.equal(R.maxpool_bwd(dpool, idx, x, scale, shift), want)


@pytest.mark.parametrize("u8", [False, True])
def test_conv1_references_match_autograd(u8):
    g = torch.Generator().manual_seed(9)
    B, H, W, C = 2, 6, 9, 5
    img = torch.randint(0, 256, (B, H, W), generator=g).to(torch.uint8) if u8 else torch.rand(B, H, W, generator=g, dtype=F64)
    stats = R.img_stats(img.reshape(B, -1), 1e-5)
    x = R.pixels(img, F64)
    assert _close(R.whiten(img, stats), F.layer_norm(x, (H, W), None, None, 1e-5), 1e-10)
    w = torch.randn(C, 9, generator=g, dtype=F64)
    wr = w.clone().requires_grad_(True)
    y = F.conv2d(R.whiten(img, stats)[:, None], wr.view(C, 1, 3, 3), stride=(2, 1), padding=1).permute(0, 2, 3, 1)
    out, col = R.conv1_fwd(img, stats, w)
    assert _close(out, y.detach()) and _close(col[:, 0].sum(0), out.sum((0, 1, 2)), 1e-10)
    assert _close(col[:, 1].sum(0), (out * out).sum((0, 1, 2)), 1e-10) and col.shape == (B * H // 2, 2, C)
    dy = torch.randn(B, H // 2, W, C, generator=g, dtype=F64)
    (y * dy).sum().backward()
    assert _close(R.conv1_wgrad(img, stats, dy), wr.grad, 1e-10)
    # the whole first stage: autograd == the unfused chain through the scan's bytes
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    Hp = R.pooled_rows(H // 2)
    dpool = torch.randn(B, Hp, W, C, generator=g, dtype=F64)
    dw, dgamma, dbeta, yc, mean, rstd = R.conv1_chain_autograd(img, stats, w, gamma, beta, dpool, 1e-5)
    scale = gamma * rstd
    _, idx = R.bn_relu_maxpool(yc, scale, beta - mean * scale)
    dw2, dgamma2, dbeta2 = R.conv1_chain_unfused(img, stats, w, gamma, mean, rstd, dpool, idx)
    assert _close(dw2, dw, 1e-8) and _close(dgamma2, dgamma, 1e-9) and _close(dbeta2, dbeta, 1e-9)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 2, 1), (2, 4, 4), (3, 10, 37)])
def test_stem_references(B, H, W, u8):
    """moments: an explicit loop over the nine zero-padded, strided taps; column statistics from the moments == conv1_fwd's
    summed over its rows; the fused forward == ATen's conv2d -> relu -> max_pool2d; the float16 bound really bounds a
    float64 evaluation over float16-rounded operands"""
    g = torch.Generator().manual_seed(B * 100 + H + W)
    C = 6
    img = torch.randint(0, 256, (B, H, W), generator=g).to(torch.uint8) if u8 else torch.rand(B, H, W, generator=g, dtype=F64)
    stats = R.img_stats(img.reshape(B, -1), 1e-5)
    w = torch.randn(C, 9, generator=g, dtype=F64) * 0.3
    xw = F.pad(R.whiten(img, stats), (1, 1, 1, 1))
    Hc = H // 2
    taps = torch.stack([xw[:, r:r + 2 * Hc:2, c:c + W] for r in range(3) for c in range(3)])      # [9][B][Hc][W]
    X, Rm = R.stem_moments(img, stats)
    assert X.shape == (9,) and Rm.shape == (9, 9)
    assert _close(X, taps.sum((1, 2, 3)), 1e-12) and _close(Rm, torch.einsum("tbhw,ubhw->tu", taps, taps), 1e-12)
    out, col = R.conv1_fwd(img, stats, w)
    cs = R.stem_colstats(img, stats, w)
    assert cs.shape == (2, C)
    assert _close(cs[0], col[:, 0].sum(0), 1e-12) and _close(cs[1], col[:, 1].sum(0), 1e-12)
    scale, shift = torch.randn(C, generator=g, dtype=F64) + 1, torch.randn(C, generator=g, dtype=F64) * 0.5
    y, idx = R.stem_fwd(img, stats, w, scale, shift)
    z = torch.relu(out * scale + shift).permute(0, 3, 1, 2)
    assert torch.equal(y, F.max_pool2d(z, 3, stride=(2, 1), padding=1).permute(0, 2, 3, 1))
    assert y.shape == (B, R.pooled_rows(Hc), W, C) and idx.dtype == torch.uint8 and torch.equal(idx == 15, ~(y > 0))
    bound = R.stem_f16_bound(img, stats, w, scale)
    assert bound.shape == out.shape
    w16 = (w * scale[:, None]).to(torch.float16).to(F64)
    x16 = R.whiten(img, stats).to(torch.float16).to(F64)
    u16 = F.conv2d(x16[:, None], w16.view(C, 1, 3, 3), stride=(2, 1), padding=1).permute(0, 2, 3, 1) + shift
    d = (u16 - (out * scale + shift)).abs()
    assert (d <= bound * (1 + 2.0 ** -10) + 1e-12).all()
    assert B * H * W < 32 or float((d / bound.clamp_min(1e-30)).max()) > 0.05      # and is no idle bound


def test_e32_and_gate_helpers():
    x = torch.randn(64, 64, dtype=F64)
    (ref,), (err,) = R.e32(lambda a: a @ a, [x])
    assert ref.dtype == F64 and 1e-9 < err < 1e-5
    ok, obs = R.gate_check("self", ref, ref, err, False)
    assert ok and obs == 0.0
    ok, _ = R.gate_check("off", ref + 100 * err * ref.abs().max(), ref, err, False)
    assert not ok
    ok, _ = R.gate_check("bf16", ref.bfloat16(), ref, err, True)
    assert ok
