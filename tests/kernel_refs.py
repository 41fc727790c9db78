"""Plain torch statements of the HBM-bound kernels' operations, in the layout the kernels use (NHWC activations,
[rows][D] tokens), written from include/htrvt.h and the reference model's semantics -- not from the kernels.

Every function computes in the dtype of its floating-point inputs and on their device: called with float64 tensors it is
the yardstick, called with float32 tensors it is "the same operation evaluated in float32", whose distance from the
yardstick (`e32`) scales the gates of the GPU parity tests.  No GPU is needed to import or run this module
(tests/test_kernel_refs_cpu.py checks it against torch's own operators and float64 autograd).
"""
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------ comparison helpers
def e32(fn, args, pick=None):
    """float32 evaluation error of `fn` on these very inputs, per output: max |fn(float32) - fn(float64)| / max |fn(float64)|.
    args: tensors (floating ones are cast, others passed as they are) and plain values; fn returns a tensor or a tuple.
    Returns (tuple of float64 outputs, tuple of errors)."""
    def cast(a, dtype):
        return a.to(dtype) if isinstance(a, torch.Tensor) and a.is_floating_point() else a
    out64 = fn(*[cast(a, torch.float64) for a in args])
    out32 = fn(*[cast(a, torch.float32) for a in args])
    if isinstance(out64, torch.Tensor):
        out64, out32 = (out64,), (out32,)
    errs = []
    for a, b in zip(out64, out32):
        if a is None:
            errs.append(0.0)
            continue
        errs.append(float((b.double() - a).abs().max() / a.abs().max().clamp_min(1e-300)))
    return tuple(out64), tuple(errs)


def gate_check(name, got, ref, err32, bf16_out, factor=8.0):
    """|got - ref| <= factor * err32 * max|ref|  (+ one bfloat16 ulp of the reference value, 2^-8 |ref|, for a bfloat16
    output: the kernel rounds once from float32), per element.  Prints E32 / gate / observed, returns (ok, observed)."""
    ref = ref.double()
    scale = float(ref.abs().max().clamp_min(1e-300))
    d = (got.double() - ref).abs()
    tol = factor * err32 * scale + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)
    obs = float(d.max() / scale)
    worst = float((d - tol).max())
    gate = factor * err32 + (2.0 ** -8 if bf16_out else 0.0)
    print(f"  {name}: E32 {err32:.2e}  gate {gate:.2e}  observed {obs:.2e}")
    return worst <= 0.0, obs


# ------------------------------------------------------------------ LayerNorm (HTR_VT.py:68,75,169: nn.LayerNorm, eps 1e-6)
def layernorm_fwd(x, gamma, beta, eps):
    """x [rows][D] -> y, mean [rows], rstd [rows] (biased variance)"""
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1) + eps)
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, dres=None):
    """-> dx (+ dres), dgamma [D], dbeta [D]; mean / rstd are the forward's saved statistics"""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    dx = rstd[:, None] * (g - m1 - xh * m2)
    if dres is not None:
        dx = dx + dres
    return dx, (dy * xh).sum(0), dy.sum(0)


# ------------------------------------------------------------------ row softmax (HTR_VT.py:32-36)
def softmax_rows(s, bias=None):
    """s [rows][n]; bias [bias_rows][n] or None, score row r takes bias row r % bias_rows"""
    if bias is not None:
        r = torch.arange(s.shape[0], device=s.device) % bias.shape[0]
        s = s + bias[r]
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd_rows(p, dp, scale):
    return scale * p * (dp - (dp * p).sum(-1, keepdim=True))


# ------------------------------------------------------------------ param-free LN over all N*C logits of a sample
def seq_whiten_fwd(x, eps):
    """x [B][NC] -> y [B][NC], stats [B][2] = {mean, rstd}"""
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return xc * rstd, torch.cat([mean, rstd], dim=1)


def seq_whiten_bwd(dy, y, stats):
    """dy, y [B][NC] -> dx [B][NC] = rstd * (dy - mean(dy) - y * mean(dy * y))"""
    return stats[:, 1:2] * (dy - dy.mean(-1, keepdim=True) - y * (dy * y).mean(-1, keepdim=True))


# ------------------------------------------------------------------ BatchNorm (resnet18.py:27-37)
def bn_finalize(partial, count, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """partial [rows][2][C] = per-row (sum, sum of squares) -> scale, shift, mean, rstd, new running_mean, new running_var
    (None without running statistics).  running_var takes the unbiased variance; count == 1 has none (torch: NaN) and
    keeps the biased one -- the rule include/htrvt.h states."""
    s = partial.sum(0)
    mean = s[0] / count
    var = (s[1] / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    rm = rv = None
    if running_mean is not None:
        unb = var * count / (count - 1.0) if count > 1 else var
        rm = (1.0 - momentum) * running_mean + momentum * mean
        rv = (1.0 - momentum) * running_var + momentum * unb
    return scale, shift, mean, rstd, rm, rv


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps):
    rstd = 1.0 / torch.sqrt(running_var + eps)
    scale = gamma * rstd
    return scale, beta - running_mean * scale, rstd


def bn_apply(x, scale, shift, res=None, rscale=None, rshift=None, relu=False):
    """x [npix][C]; residual modes: none / identity / residual with its own coefficients"""
    y = x * scale + shift
    if res is not None:
        y = y + (res if rscale is None else res * rscale + rshift)
    return torch.relu(y) if relu else y


def bn_bwd_sums(dy, yact, x, mean, rstd):
    """g = dy * (yact > 0) (yact None: g = dy) -> g, sum g [C], sum g * xhat [C]"""
    g = dy if yact is None else torch.where(yact > 0, dy, torch.zeros_like(dy))
    return g, g.sum(0), (g * (x - mean) * rstd).sum(0)


def bn_bwd_coef(s1, s2, count, gamma, mean, rstd):
    """[3][C] coefficients of dx = cA * g + cB * x + cC; count <= 0: eval mode (statistics are constants)"""
    cA = gamma * rstd
    if count <= 0:
        return torch.stack([cA, torch.zeros_like(cA), torch.zeros_like(cA)])
    cB = -gamma * rstd * rstd * s2 / count
    cC = -gamma * rstd * s1 / count - cB * mean
    return torch.stack([cA, cB, cC])


def bn_bwd(dy, yact, x, mean, rstd, gamma, count):
    """closed form: dx, dgamma, dbeta, g"""
    g, s1, s2 = bn_bwd_sums(dy, yact, x, mean, rstd)
    if count <= 0:
        return gamma * rstd * g, s2, s1, g
    xh = (x - mean) * rstd
    return gamma * rstd * (g - s1 / count - xh * s2 / count), s2, s1, g


def bn_bwd_autograd(dy, x, gamma, beta, eps):
    """train-mode F.batch_norm under autograd: dx, dgamma, dbeta, and the batch mean / rstd it used"""
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.batch_norm(xr.t()[None], None, None, gr, br, True, 0.0, eps)[0].t()      # [npix][C] -> [1][C][npix]
    (y * dy).sum().backward()
    mean = x.mean(0)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(0) + eps)
    return xr.grad, gr.grad, br.grad, mean, rstd


# ------------------------------------------------------------------ relu(bn(x)) -> max_pool2d(3, (2,1), 1) with arg-max bytes
def pooled_rows(H):
    return (H - 1) // 2 + 1


def bn_relu_maxpool(x, scale=None, shift=None):
    """x [B][H][W][C] -> y [B][Ho][W][C], idx uint8: 3 * row + col of the FIRST maximum of the window in (row, column)
    scan order; 15 where a scale is given and the pooled value is not > 0 (the ReLU is closed: no gradient).
    An explicit scan over the nine window cells, strict > so that the first maximum wins."""
    B, H, W, C = x.shape
    Ho = pooled_rows(H)
    v = x if scale is None else torch.relu(x * scale + shift)
    pad = torch.full((B, H + 2, W + 2, C), float("-inf"), dtype=v.dtype, device=v.device)
    pad[:, 1:H + 1, 1:W + 1] = v
    best = torch.full((B, Ho, W, C), float("-inf"), dtype=v.dtype, device=v.device)
    idx = torch.zeros((B, Ho, W, C), dtype=torch.uint8, device=v.device)
    for r in range(3):
        for c in range(3):
            cell = pad[:, r:r + 2 * Ho:2, c:c + W]
            take = cell > best
            best = torch.where(take, cell, best)
            idx = torch.where(take, torch.full_like(idx, 3 * r + c), idx)
    if scale is not None:
        idx = torch.where(best > 0, idx, torch.full_like(idx, 15))
    return best, idx


def maxpool_bwd(dpool, idx, x, scale=None, shift=None):
    """scatter dpool through the bytes (a byte outside 0..8 passes nothing), then the ReLU mask x*scale+shift > 0"""
    B, H, W, C = x.shape
    Ho = pooled_rows(H)
    gp = torch.zeros((B, H + 2, W + 2, C), dtype=dpool.dtype, device=dpool.device)
    for r in range(3):
        for c in range(3):
            gp[:, r:r + 2 * Ho:2, c:c + W] += torch.where(idx == 3 * r + c, dpool, torch.zeros_like(dpool))
    g = gp[:, 1:H + 1, 1:W + 1]
    if scale is not None:
        g = torch.where(x * scale + shift > 0, g, torch.zeros_like(g))
    return g.contiguous()


# ------------------------------------------------------------------ image statistics and conv1 (HTR_VT.py:224, resnet18.py:74)
def pixels(img, dtype):
    """float image as it is; uint8 image as value / 255 (torchvision ToTensor)"""
    return img.to(dtype) / 255.0 if img.dtype == torch.uint8 else img.to(dtype)


def img_stats(img, eps, dtype=torch.float64):
    """img [B][HW] -> stats [B][2] = {mean, rstd} (param-free LayerNorm, biased variance)"""
    x = pixels(img, dtype)
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return torch.cat([mean, rstd], dim=1)


def whiten(img, stats):
    return (pixels(img, stats.dtype) - stats[:, 0, None, None]) * stats[:, 1, None, None]


def conv1_fwd(img, stats, w):
    """img [B][H][W], stats [B][2], w [C][9] -> out [B][H/2][W][C] (NHWC), colstats [B*H/2][2][C] = per output row
    (sum, sum of squares) over its W pixels"""
    C = w.shape[0]
    out = F.conv2d(whiten(img, stats)[:, None], w.view(C, 1, 3, 3), stride=(2, 1), padding=1).permute(0, 2, 3, 1).contiguous()
    col = torch.stack([out.sum(2), (out * out).sum(2)], dim=2)          # [B][Ho][2][C]
    return out, col.reshape(-1, 2, C)


def stem_moments(img, stats):
    """-> X [9], R [9][9]: the sum of each of the nine whitened, zero-padded taps over all conv output positions
    (stride (2,1), pad 1) and the sums of their pairwise products"""
    taps = F.unfold(whiten(img, stats)[:, None], 3, padding=1, stride=(2, 1))     # [B][9][Ho*W]
    return taps.sum((0, 2)), torch.einsum("btp,bup->tu", taps, taps)


def stem_colstats(img, stats, w):
    """-> [2][C] = (sum, sum of squares) of the conv1 output per channel over the whole batch, from the image moments
    alone: sum y_c = w_c . X, sum y_c^2 = w_c^T R w_c"""
    X, Rm = stem_moments(img, stats)
    return torch.stack([w @ X, torch.einsum("ct,tu,cu->c", w, Rm, w)])


def stem_fwd(img, stats, w, scale, shift):
    """conv1 -> BatchNorm (scale, shift) -> ReLU -> max-pool: y [B][Hp][W][C], idx uint8 as bn_relu_maxpool"""
    return bn_relu_maxpool(conv1_fwd(img, stats, w)[0], scale, shift)


def stem_f16_bound(img, stats, w, scale):
    """-> [B][H/2][W][C]: bound on the error of the BatchNorm output when the scaled weights w[c][t] * scale[c] and the
    whitened taps x_t are each rounded to float16 (relative 2^-11 each, so 2^-10 per product, second order dropped):
    2^-10 * sum_t |w[c][t] scale[c]| |x_t|, the same convolution over absolute values"""
    C = w.shape[0]
    aw = (w * scale[:, None]).abs().view(C, 1, 3, 3)
    return 2.0 ** -10 * F.conv2d(whiten(img, stats).abs()[:, None], aw, stride=(2, 1), padding=1).permute(0, 2, 3, 1).contiguous()


def conv1_wgrad(img, stats, dy):
    """dy [B][H/2][W][C] -> dw [C][9] = sum over pixels of dy * whitened tap"""
    B, Ho, W, C = dy.shape
    taps = F.unfold(whiten(img, stats)[:, None], 3, padding=1, stride=(2, 1))     # [B][9][Ho*W]
    return torch.einsum("bpc,btp->ct", dy.reshape(B, Ho * W, C), taps)


def conv1_chain_autograd(img, stats, w, gamma, beta, dpool, eps):
    """conv1 -> BatchNorm(train) -> ReLU -> max_pool2d(3, (2,1), 1) under autograd: dw [C][9], dgamma, dbeta, and the
    conv output (NHWC), batch mean / rstd of the BatchNorm"""
    C = w.shape[0]
    wr, gr, br = w.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.conv2d(whiten(img, stats)[:, None], wr.view(C, 1, 3, 3), stride=(2, 1), padding=1)
    z = torch.relu(F.batch_norm(y, None, None, gr, br, True, 0.0, eps))
    p = F.max_pool2d(z, 3, stride=(2, 1), padding=1)
    (p * dpool.permute(0, 3, 1, 2)).sum().backward()
    yd = y.detach()
    mean = yd.mean((0, 2, 3))
    rstd = 1.0 / torch.sqrt(((yd - mean[None, :, None, None]) ** 2).mean((0, 2, 3)) + eps)
    return wr.grad, gr.grad, br.grad, yd.permute(0, 2, 3, 1).contiguous(), mean, rstd


def conv1_chain_unfused(img, stats, w, gamma, mean, rstd, dpool, idx):
    """the same gradients as the unfused kernels form them: max-pool backward through the given bytes, BatchNorm backward
    with the given batch statistics, conv1 weight gradient"""
    y, _ = conv1_fwd(img, stats, w)
    B, Hc, W, C = y.shape
    g = maxpool_bwd(dpool, idx, y)          # byte 15 already carries the ReLU mask of the arg-max element
    dx, dgamma, dbeta, _ = bn_bwd(g.reshape(-1, C), None, y.reshape(-1, C), mean, rstd, gamma, float(B * Hc * W))
    return conv1_wgrad(img, stats, dx.reshape(B, Hc, W, C)), dgamma, dbeta
