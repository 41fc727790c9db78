"""Plain torch statements of the convolutional token mixer (ConvLocalMixer1D of the macaron forks), in the layout the
kernels use: token rows [B*N][D], the depthwise convolution running along the tokens of one image with zero padding.
Written from include/htrvt.h and the fork's module, not from the kernels.  Like tests/kernel_refs.py every function
computes in the dtype of its inputs: float64 is the yardstick, float32 "the same operation in float32" for kernel_refs.e32.
No GPU is needed (tests/test_conv_mixer_cpu.py checks this module against arrays the fork's own module produced).
"""
import torch
import torch.nn.functional as F


def glu(u):
    """u [rows][2D] -> g [rows][D] = value half * sigmoid(gate half)"""
    D = u.shape[1] // 2
    return u[:, :D] * torch.sigmoid(u[:, D:])


def dwconv_tokens(g, w, B, N):
    """g [B*N][D], w [D][k] -> c[b][n][d] = sum_j w[d][j] * g[b][n + j - k//2][d], zero outside 0 .. N-1 of image b.
    An explicit sum over the taps on a per-image zero-padded copy (no conv operator)."""
    D, k = w.shape
    p = k // 2
    pad = torch.zeros(B, N + 2 * p, D, dtype=g.dtype, device=g.device)
    pad[:, p:p + N] = g.view(B, N, D)
    c = torch.zeros(B, N, D, dtype=g.dtype, device=g.device)
    for j in range(k):
        c = c + w[:, j] * pad[:, j:j + N]
    return c.reshape(B * N, D)


def silu(z):
    return z * torch.sigmoid(z)


def glu_dwconv(u, w, B, N):
    """step 3-4 without the bias: c [B*N][D]"""
    return dwconv_tokens(glu(u), w, B, N)


def bn_train(c, gamma, beta, eps, momentum, running_mean, running_var):
    """train-mode BatchNorm1d over the rows of c -> z, mean, rstd, new running_mean, new running_var (unbiased)"""
    n = c.shape[0]
    mean = c.mean(0)
    var = ((c - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (c - mean) * rstd * gamma + beta
    rm = (1.0 - momentum) * running_mean + momentum * mean
    rv = (1.0 - momentum) * running_var + momentum * var * n / (n - 1.0)
    return z, mean, rstd, rm, rv


def bn_eval(c, gamma, beta, eps, running_mean, running_var):
    return (c - running_mean) / torch.sqrt(running_var + eps) * gamma + beta


def mixer_core(u, w, B, N, gamma=None, beta=None, running_mean=None, running_var=None, training=False, eps=1e-5,
               momentum=0.1, conv_bias=None):
    """steps 3-6: u [B*N][2D] -> (s [B*N][D], c, new running_mean, new running_var); gamma None: no BatchNorm, z = c +
    conv_bias.  c is the convolution without the bias."""
    c = glu_dwconv(u, w, B, N)
    rm = rv = None
    if gamma is None:
        z = c if conv_bias is None else c + conv_bias
    elif training:
        z, _, _, rm, rv = bn_train(c, gamma, beta, eps, momentum, running_mean, running_var)
    else:
        z = bn_eval(c, gamma, beta, eps, running_mean, running_var)
    return silu(z), c, rm, rv


def mixer_core_bwd(ds, u, w, B, N, gamma=None, beta=None, running_mean=None, running_var=None, training=False, eps=1e-5,
                   conv_bias=None):
    """backward of mixer_core by autograd: dict of du, dw and (where they exist) dgamma, dbeta, dbias"""
    leaves = {"du": u, "dw": w, "dgamma": gamma, "dbeta": beta, "dbias": conv_bias}
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items() if v is not None}
    s = mixer_core(leaves["du"], leaves["dw"], B, N, leaves.get("dgamma"), leaves.get("dbeta"), running_mean, running_var,
                   training, eps, 0.1, leaves.get("dbias"))[0]
    grads = torch.autograd.grad((s * ds).sum(), list(leaves.values()))
    return dict(zip(leaves.keys(), grads))


def layernorm(x, gamma, beta, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def mixer_module(sd, x, training, keep=None, drop_p=0.0, eps=1e-5, momentum=0.1):
    """the whole module on a state_dict of the fork's names (12 entries with BatchNorm, 9 without): x [B][N][D] ->
    (y, new running_mean, new running_var).  keep: the dropout mask [B*N][D] of 0 / 1 (None: no dropout), applied as
    o * keep / (1 - drop_p)."""
    B, N, D = x.shape
    t = layernorm(x.reshape(B * N, D), sd["norm.weight"], sd["norm.bias"], 1e-5)
    u = t @ sd["pw_in.weight"].t() + sd["pw_in.bias"]
    use_bn = "bn.weight" in sd
    s, _, rm, rv = mixer_core(u, sd["dwconv.weight"][:, 0], B, N, sd.get("bn.weight"), sd.get("bn.bias"),
                              sd.get("bn.running_mean"), sd.get("bn.running_var"), training and use_bn, eps, momentum,
                              sd.get("dwconv.bias"))
    o = s @ sd["pw_out.weight"].t() + sd["pw_out.bias"]
    if keep is not None:
        o = o * keep / (1.0 - drop_p)
    return x + o.view(B, N, D), rm, rv


def mixer_module_grads(sd, x, dy, training, keep=None, drop_p=0.0):
    """autograd through mixer_module: (dx, {parameter name: gradient})"""
    names = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    xr = x.detach().clone().requires_grad_(True)
    full = dict(sd)
    full.update(leaves)
    y = mixer_module(full, xr, training, keep, drop_p)[0]
    grads = torch.autograd.grad((y * dy).sum(), [xr] + list(leaves.values()))
    return grads[0], dict(zip(names, grads[1:]))


def fork_conv(g, w, B, N, bias=None):
    """the fork's own route for step 4 -- transpose to [B][D][N], F.conv1d(groups=D), transpose back -- for the CPU test of
    dwconv_tokens"""
    D, k = w.shape
    y = F.conv1d(g.view(B, N, D).transpose(1, 2), w[:, None], bias, padding=k // 2, groups=D)
    return y.transpose(1, 2).reshape(B * N, D)


# ------------------------------------------------------------------ the backward as the kernels stage it
def silu_bwd(ds, z):
    sg = torch.sigmoid(z)
    return ds * sg * (1 + z * (1 - sg))


def affine(c, scale, shift):
    """z = c * scale + shift; None stands for 1 / 0"""
    z = c if scale is None else c * scale
    return z if shift is None else z + shift


def bwd_sums(ds, c, scale, shift, mean, rstd):
    """(sum dz, sum dz * xhat) over the rows, dz = ds * silu'(c * scale + shift)"""
    dz = silu_bwd(ds, affine(c, scale, shift))
    return dz.sum(0), (dz * (c - mean) * rstd).sum(0)


def core_bwd(ds, c, u, w, B, N, scale, shift, coef=None):
    """closed form of the main backward launch: dc = coef[0] * dz + coef[1] * c + coef[2] (None: dz), dg = dc convolved with
    the flipped taps, the GLU backward -> du [B*N][2D], dw [D][k], sum dc [D]"""
    D, k = w.shape
    p = k // 2
    dz = silu_bwd(ds, affine(c, scale, shift))
    dc = dz if coef is None else coef[0] * dz + coef[1] * c + coef[2]
    dg = dwconv_tokens(dc, w.flip(1), B, N)
    a, sb = u[:, :D], torch.sigmoid(u[:, D:])
    du = torch.cat([dg * sb, dg * a * sb * (1 - sb)], 1)
    pad = torch.zeros(B, N + 2 * p, D, dtype=u.dtype, device=u.device)
    pad[:, p:p + N] = (a * sb).view(B, N, D)
    dw = torch.stack([(dc.view(B, N, D) * pad[:, j:j + N]).sum((0, 1)) for j in range(k)], 1)
    return du, dw, dc.sum(0)
