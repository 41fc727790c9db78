"""Plain torch statements of the VAN forks' operators (csrc/van.hip) in the layout the kernels use -- NHWC activations
[B][H][W][C], depthwise weights [C][kh * kw] -- and of the two modules composed from them.

Written from include/htrvt.h and the fork's modules (model_sgm_mms_attach_van/model/HTR_VT.py: LargeKernelAttention,
VANBlock, VANHeightReducer, HorizontalMixer), not from the kernels.  Like tests/kernel_refs.py every function computes in
the dtype of its floating-point inputs: float64 is the yardstick, float32 "the same operation in float32" whose distance
from the yardstick (kernel_refs.e32) scales the gates of the GPU tests.  tests/test_van_cpu.py checks the convolutions
against torch.nn.functional.conv2d and its autograd, the closed-form backward statements against autograd through the
forward ones, and the composed modules against tests/golden/van.npz (the fork's own modules in float64)."""
import math

import torch

import kernel_refs as R

EPS, MOM = 1e-5, 0.1           # nn.BatchNorm2d defaults, as the fork builds it


# ------------------------------------------------------------------ depthwise convolution
def _shift(x, dh, dw):
    """out[b][h][w] = x[b][h + dh][w + dw], zero where that leaves the image"""
    B, H, W, C = x.shape
    out = torch.zeros_like(x)
    h0, h1, w0, w1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
    if h0 < h1 and w0 < w1:
        out[:, h0:h1, w0:w1] = x[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
    return out


def _taps(kh, kw, dil):
    for i in range(kh):
        for j in range(kw):
            yield i * kw + j, (i - kh // 2) * dil, (j - kw // 2) * dil


def dwconv(x, w, kh, kw, dil):
    """y[b][h][w][c] = sum_ij w[c][i kw + j] x[b][h + (i - kh/2) dil][w + (j - kw/2) dil][c], zero padding per image"""
    y = torch.zeros_like(x)
    for t, dh, dw in _taps(kh, kw, dil):
        y = y + w[:, t] * _shift(x, dh, dw)
    return y


def dwconv_bwd_input(dy, w, kh, kw, dil, add=None):
    """dy convolved with the flipped taps (+ add)"""
    dx = torch.zeros_like(dy) if add is None else add.clone()
    for t, dh, dw in _taps(kh, kw, dil):
        dx = dx + w[:, t] * _shift(dy, -dh, -dw)
    return dx


def dwconv_bwd_weight(x, dy, kh, kw, dil):
    """d w [C][kh kw] = sum_bhw dy * shifted x"""
    return torch.stack([(dy * _shift(x, dh, dw)).sum((0, 1, 2)) for _, dh, dw in _taps(kh, kw, dil)], dim=1)


def conv2d_weight(w, kh, kw):
    """[C][kh kw] -> the Conv2d parameter [C][1][kh][kw] (the same memory)"""
    return w.reshape(w.shape[0], 1, kh, kw)


# ------------------------------------------------------------------ passes over [rows][C]
def moments(x):
    """one partial row [1][2][C] = (sum x, sum x^2)"""
    return torch.stack([x.sum(0), (x * x).sum(0)])[None]


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def affine(x, scale=None, shift=None):
    z = x if scale is None else x * scale
    return z if shift is None else z + shift


def gate_fwd(a, p, scale, shift):
    return a * affine(p, scale, shift)


def gate_bwd(dg, a, p, scale, shift):
    """-> da (the gate's first factor only), dz (the gradient of the BatchNorm output)"""
    return dg * affine(p, scale, shift), dg * a


def bn_res_gelu_fwd(x, scale, shift, res=None):
    z = affine(x, scale, shift)
    return gelu(z if res is None else res + z)


def bn_res_gelu_bwd(dy, x, scale, shift, res=None):
    z = affine(x, scale, shift)
    return dy * gelu_grad(z if res is None else res + z)


def hpool_fwd(x):
    return x.mean(1)


def hpool_bwd(d, H):
    return (d / H)[:, None].expand(-1, H, -1, -1).contiguous()


# ------------------------------------------------------------------ the modules, from a state_dict with the fork's names
def _bn(x, sd, pre, training, buffers):
    """BatchNorm2d over rows [rows][C] -> (scale, shift); training: batch statistics, the new buffers recorded"""
    gamma, beta, rm, rv = sd[pre + "weight"], sd[pre + "bias"], sd[pre + "running_mean"], sd[pre + "running_var"]
    if not training:
        scale, shift, _ = R.bn_eval_coeffs(gamma, beta, rm, rv, EPS)
        return scale, shift
    scale, shift, _, _, nrm, nrv = R.bn_finalize(moments(x), float(x.shape[0]), gamma, beta, EPS, MOM, rm, rv)
    buffers[pre + "running_mean"], buffers[pre + "running_var"] = nrm.detach(), nrv.detach()
    buffers[pre + "num_batches_tracked"] = sd[pre + "num_batches_tracked"] + 1
    return scale, shift


def _pw(x, sd, pre):
    """1x1 convolution on rows"""
    C = x.shape[1]
    y = x @ sd[pre + "weight"].reshape(-1, C).t()
    return y + sd[pre + "bias"] if pre + "bias" in sd else y


def _dw(x, sd, pre, dil):
    w = sd[pre + "weight"]
    kh, kw = w.shape[-2:]
    return dwconv(x, w.reshape(w.shape[0], kh * kw), kh, kw, dil)


def lka(a, sd, pre, training, buffers):
    """a [B][H][W][C] -> rows [B H W][C]"""
    C = a.shape[-1]
    p = _pw(_dw(_dw(a, sd, pre + "dw.", 1), sd, pre + "dwd.", 3).reshape(-1, C), sd, pre + "pw.")
    return gate_fwd(a.reshape(-1, C), p, *_bn(p, sd, pre + "bn.", training, buffers))


def van_block(x, sd, pre, training, buffers, taps=None):
    """taps (a dict, or None): receives the norm's input rows under the name of proj2.bias, with their gradient retained --
    the terms whose sum is that bias's gradient"""
    C = x.shape[-1]
    a = gelu(_pw(x.reshape(-1, C), sd, pre + "proj1."))
    q = _pw(lka(a.reshape(x.shape), sd, pre + "lka.", training, buffers), sd, pre + "proj2.")
    if taps is not None and q.requires_grad:
        q.retain_grad()
        taps[pre + "proj2.bias"] = q
    scale, shift = _bn(q, sd, pre + "norm.", training, buffers)
    return R.bn_apply(q, scale, shift, res=x.reshape(-1, C)).reshape(x.shape)


def reducer(sd, x, training, depth, pre="", taps=None):
    """VANHeightReducer: x (B, C, H, W) -> (y (B, C, 1, W), {buffer name: new value} of a train forward)"""
    buffers = {}
    t = x.permute(0, 2, 3, 1)
    for i in range(depth):
        t = van_block(t, sd, f"{pre}blocks.{i}.", training, buffers, taps)
    return hpool_fwd(t)[:, None].permute(0, 3, 1, 2), buffers


def hmixer(sd, x, training, pre=""):
    """HorizontalMixer: x (B, C, 1, W) -> (y, new buffers)"""
    buffers = {}
    t = x.permute(0, 2, 3, 1)
    C = t.shape[-1]
    p = _pw(_dw(t, sd, pre + "dw.", 1).reshape(-1, C), sd, pre + "pw.")
    scale, shift = _bn(p, sd, pre + "bn.", training, buffers)
    y = bn_res_gelu_fwd(p, scale, shift, res=t.reshape(-1, C))
    return y.reshape(t.shape).permute(0, 3, 1, 2), buffers


def module_grads(fn, sd, x, dy):
    """backward of sum(fn(sd, x)[0] * dy) in train mode -> (dx, {parameter name: gradient})"""
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    xr = x.clone().requires_grad_(True)
    y, _ = fn({**sd, **leaves}, xr)
    (y * dy).sum().backward()
    return xr.grad, {k: v.grad for k, v in leaves.items()}
