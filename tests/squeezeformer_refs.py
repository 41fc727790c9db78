"""Plain torch statements of the convolutional forks' blocks (ConvModule, FeedForward, SqueezeExcite1D, Downsample1D,
Upsample1D, ConformerBlock, SqueezeConformerBlock, SqueezeFormerEncoder), in the layout the kernels use: token rows
[B*N][D].  Written from include/htrvt.h and the mathematics of the forks' modules, not from the kernels.  Like
tests/kernel_refs.py every function computes in the dtype of its inputs: float64 is the yardstick, float32 "the same
operation in float32" for kernel_refs.e32.  No GPU is needed (tests/test_squeezeformer_cpu.py checks this module against
arrays the fork's own modules produced)."""
import torch

from conv_mixer_refs import dwconv_tokens, glu, layernorm, silu, silu_bwd  # noqa: F401


# ------------------------------------------------------------------ the GroupNorm mixer, stage by stage
def gn_conv(u, w, bias, B, N):
    """c [B*N][C] = dwconv(glu(u)) + bias"""
    return dwconv_tokens(glu(u), w, B, N) + bias


def gn_stats(c, B, N, eps):
    """(mean [B], rstd [B]) over all C * N values of each image, biased variance"""
    x = c.view(B, -1)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + eps)


def _per_row(v, N):
    """[B] -> [B*N][1]"""
    return v.repeat_interleave(N)[:, None]


def gn_xhat(c, mean, rstd, N):
    return (c - _per_row(mean, N)) * _per_row(rstd, N)


def gn_act(c, mean, rstd, gamma, beta, N):
    return silu(gn_xhat(c, mean, rstd, N) * gamma + beta)


def gn_mixer(u, w, bias, gamma, beta, B, N, eps=1e-5):
    """u [B*N][2C] -> s [B*N][C], end to end"""
    c = gn_conv(u, w, bias, B, N)
    mean, rstd = gn_stats(c, B, N, eps)
    return gn_act(c, mean, rstd, gamma, beta, N)


def gn_bwd_sums(ds, c, mean, rstd, gamma, beta, B, N):
    """per channel (sum dz, sum dz xhat) [C] and per image (sum gamma dz, sum gamma dz xhat) [B], dz = ds * silu'(z)"""
    xh = gn_xhat(c, mean, rstd, N)
    dz = silu_bwd(ds, xh * gamma + beta)
    return dz.sum(0), (dz * xh).sum(0), (gamma * dz).view(B, -1).sum(1), (gamma * dz * xh).view(B, -1).sum(1)


def gn_core_bwd(ds, c, u, w, mean, rstd, gamma, beta, m1, m2, B, N):
    """closed form of the main backward launch: dc = rstd_b (gamma dz - m1_b - xhat m2_b), dg = dc convolved with the flipped
    taps, the GLU backward -> du [B*N][2C], dw [C][k], db [C] = sum dc"""
    C, k = w.shape
    p = k // 2
    xh = gn_xhat(c, mean, rstd, N)
    dz = silu_bwd(ds, xh * gamma + beta)
    dc = _per_row(rstd, N) * (gamma * dz - _per_row(m1, N) - xh * _per_row(m2, N))
    dg = dwconv_tokens(dc, w.flip(1), B, N)
    a, sb = u[:, :C], torch.sigmoid(u[:, C:])
    du = torch.cat([dg * sb, dg * a * sb * (1 - sb)], 1)
    pad = torch.zeros(B, N + 2 * p, C, dtype=u.dtype, device=u.device)
    pad[:, p:p + N] = (a * sb).view(B, N, C)
    dw = torch.stack([(dc.view(B, N, C) * pad[:, j:j + N]).sum((0, 1)) for j in range(k)], 1)
    return du, dw, dc.sum(0)


def grads_of(fn, ds, *leaves):
    """autograd through fn(*leaves): the gradients of sum(fn * ds)"""
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    return torch.autograd.grad((fn(*leaves) * ds).sum(), leaves)


# ------------------------------------------------------------------ squeeze-excite
def se_mean(x, B, N):
    return x.view(B, N, -1).mean(1)


def se_mlp(mean, w1, b1, w2, b2):
    """(pre, act, g): fc1's output, its SiLU, the gate"""
    pre = mean @ w1.t() + b1
    act = silu(pre)
    return pre, act, torch.sigmoid(act @ w2.t() + b2)


def se_scale(x, g, N):
    return x * g.repeat_interleave(N, 0)


def se(x, w1, b1, w2, b2, B, N):
    return se_scale(x, se_mlp(se_mean(x, B, N), w1, b1, w2, b2)[2], N)


def se_dg(dy, x, B, N):
    return (dy * x).view(B, N, -1).sum(1)


def se_mlp_bwd(dg, g, pre, w1, w2):
    """(dh2, dh1, dmean): the gradients at fc2's and fc1's outputs and at the mean"""
    dh2 = dg * g * (1 - g)
    dh1 = silu_bwd(dh2 @ w2, pre)
    return dh2, dh1, dh1 @ w1


def se_wgrad(dy, x):
    return dy.t() @ x, dy.sum(0)


def se_dx(dy, g, dmean, N):
    return dy * g.repeat_interleave(N, 0) + dmean.repeat_interleave(N, 0) / N


# ------------------------------------------------------------------ resampling
def down2(x, B, N):
    """the mean of tokens 2j and 2j + 1; an odd last token is dropped"""
    if N <= 1:
        return x
    n = N // 2
    v = x.view(B, N, -1)[:, :2 * n].reshape(B, n, 2, -1)
    return ((v[:, :, 0] + v[:, :, 1]) * 0.5).reshape(B * n, -1)


def up_index(n, N0):
    """source token of target i: (i * n) // N0, the integer form of F.interpolate(mode='nearest')"""
    return (torch.arange(N0) * n) // N0


def up_add(y, skip, B, n, N0):
    return y.view(B, n, -1)[:, up_index(n, N0)].reshape(B * N0, -1) + skip


# ------------------------------------------------------------------ the modules on a state_dict of the fork's names
def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def ffn(sd, x):
    return silu(x @ sd["lin1.weight"].t() + sd["lin1.bias"]) @ sd["lin2.weight"].t() + sd["lin2.bias"]


def conv_module(sd, x, B, N, keep=None, drop_p=0.0):
    """x [B*N][D] -> x + dropout(branch); keep: the dropout mask [B*N][D] of 0 / 1 (None: no dropout)"""
    t = layernorm(x, sd["layer_norm.weight"], sd["layer_norm.bias"], 1e-5)
    u = t @ sd["pointwise_conv1.weight"][:, :, 0].t() + sd["pointwise_conv1.bias"]
    s = gn_mixer(u, sd["depthwise_conv.weight"][:, 0], sd["depthwise_conv.bias"], sd["norm.weight"], sd["norm.bias"], B, N)
    o = s @ sd["pointwise_conv2.weight"][:, :, 0].t() + sd["pointwise_conv2.bias"]
    if keep is not None:
        o = o * keep / (1.0 - drop_p)
    return x + o


def attention(sd, x, B, N, heads):
    D = x.shape[1]
    qkv = (x @ sd["qkv.weight"].t() + sd["qkv.bias"]).view(B, N, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    p = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) * (D // heads) ** -0.5, -1)
    return (p @ qkv[2]).transpose(1, 2).reshape(B * N, D) @ sd["proj.weight"].t() + sd["proj.bias"]


def block(sd, x, B, N, heads, squeeze, eps):
    def ln(name, v):
        return layernorm(v, sd[name + ".weight"], sd[name + ".bias"], eps)
    x = x + 0.5 * ffn(_sub(sd, "ffn1."), ln("ffn1_norm", x))
    x = x + attention(_sub(sd, "attn."), ln("attn_norm", x), B, N, heads)
    x = conv_module(_sub(sd, "conv_module."), x, B, N)
    if squeeze:
        x = se(x, sd["se.fc1.weight"], sd["se.fc1.bias"], sd["se.fc2.weight"], sd["se.fc2.bias"], B, N)
    x = x + 0.5 * ffn(_sub(sd, "ffn2."), ln("ffn2_norm", x))
    return ln("final_norm", x)


def encoder(sd, x, B, N0, heads, eps):
    d1 = len({k.split(".")[1] for k in sd if k.startswith("stage1.")})
    d2 = len({k.split(".")[1] for k in sd if k.startswith("stage2.")})
    for i in range(d1):
        x = block(_sub(sd, f"stage1.{i}."), x, B, N0, heads, True, eps)
    skip, n = x, (N0 // 2 if N0 > 1 else N0)
    x = down2(x, B, N0)
    for i in range(d2):
        x = block(_sub(sd, f"stage2.{i}."), x, B, n, heads, True, eps)
    x = up_add(x, skip, B, n, N0)
    return layernorm(x, sd["out_norm.weight"], sd["out_norm.bias"], eps)


def run(kind, args, sd, x, eps, target=None, **kw):
    """the module of squeezeformer_cases kind on x [B][N][D] -> y [B][No][D]"""
    B, N, D = x.shape
    r = x.reshape(B * N, D)
    if kind == "ffn":
        y = ffn(sd, r)
    elif kind == "conv":
        y = conv_module(sd, r, B, N, **kw)
    elif kind == "se":
        y = se(r, sd["fc1.weight"], sd["fc1.bias"], sd["fc2.weight"], sd["fc2.bias"], B, N)
    elif kind == "down":
        y = down2(r, B, N)
    elif kind == "up":
        y = up_add(r, torch.zeros(B * target, D, dtype=x.dtype), B, N, target)
    elif kind in ("cblock", "sblock"):
        y = block(sd, r, B, N, args[1], kind == "sblock", eps)
    else:
        y = encoder(sd, r, B, N, args[1], eps)
    return y.view(B, -1, D)


def module_grads(kind, args, sd, x, dy, eps, target=None, **kw):
    """(y, dx, {parameter name: gradient}) by autograd through `run`"""
    names = [k for k, v in sd.items() if v.is_floating_point()]
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    xr = x.detach().clone().requires_grad_(True)
    y = run(kind, args, leaves, xr, eps, target, **kw)
    grads = torch.autograd.grad((y * dy).sum(), [xr] + list(leaves.values()))
    return y.detach(), grads[0], dict(zip(names, grads[1:]))
