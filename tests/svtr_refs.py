"""Plain-torch float64 statements of csrc/svtr.hip's neighbourhood attention in the kernel's own layout (token-order qkv, the
box as index arithmetic on the token map) and of the module sequences of htr-vt_amd/svtr.py.  tests/test_svtr_cpu.py anchors
them to the fork's own float64 results (tests/golden/svtr.npz); the GPU tests compare the kernels and modules with them.
Everything is differentiable by autograd."""
import torch
import torch.nn.functional as F

from swin_refs import _linear, _norm, combining


def visible(H, W, kernel):
    """vis [H*W, H*W] bool: key (y', x') is seen from query (y, x) exactly when |y - y'| <= kh // 2 and |x - x'| <= kw // 2"""
    y, x = torch.arange(H * W) // W, torch.arange(H * W) % W
    return ((y[:, None] - y[None, :]).abs() <= kernel[0] // 2) & ((x[:, None] - x[None, :]).abs() <= kernel[1] // 2)


def nbr2d_attention(qkv, B, H, W, heads, kernel):
    """qkv [B*H*W, 3*heads*hd] -> out [B*H*W, heads*hd], one slice of the zero-padded key / value maps per box offset: the
    scores are [B, H, W, heads, kh*kw], never N x N"""
    kh, kw = kernel
    ph, pw = kh // 2, kw // 2
    D = qkv.shape[1] // 3
    hd = D // heads
    q, k, v = qkv.view(B, H, W, 3, heads, hd).unbind(3)
    kp, vp = F.pad(k, (0, 0, 0, 0, pw, pw, ph, ph)), F.pad(v, (0, 0, 0, 0, pw, pw, ph, ph))
    ys, xs = torch.arange(H), torch.arange(W)
    S = []
    for dy in range(kh):
        for dx in range(kw):
            inmap = ((ys + dy - ph >= 0) & (ys + dy - ph < H))[:, None] & ((xs + dx - pw >= 0) & (xs + dx - pw < W))[None, :]
            s = (q * kp[:, dy:dy + H, dx:dx + W]).sum(-1) * hd ** -0.5
            S.append(s.masked_fill(~inmap[None, :, :, None], float("-inf")))
    P = torch.stack(S, -1).softmax(-1)
    out = 0
    for dy in range(kh):
        for dx in range(kw):
            out = out + P[..., dy * kw + dx, None] * vp[:, dy:dy + H, dx:dx + W]
    return out.reshape(B * H * W, D)


def dense_attention(qkv, B, N, heads, vis=None):
    """the fork's form: N x N scores, -inf where vis [N, N] is False (None: a global module)"""
    hd = qkv.shape[1] // 3 // heads
    q, k, v = [t.transpose(1, 2) for t in qkv.view(B, N, 3, heads, hd).unbind(2)]
    S = q @ k.transpose(-1, -2) * hd ** -0.5
    if vis is not None:
        S = S.masked_fill(~vis, float("-inf"))
    return (S.softmax(-1) @ v).transpose(1, 2).reshape(B * N, heads * hd)


def nbr2d_grads(qkv, dout, B, H, W, heads, kernel):
    """(out, dqkv) of sum(out * dout)"""
    qr = qkv.clone().requires_grad_(True)
    out = nbr2d_attention(qr, B, H, W, heads, kernel)
    (out * dout).sum().backward()
    return out.detach(), qr.grad


def mha(sd, x, H, W, heads, kernel, pre=""):
    """MultiHeadSelfAttention on x [B, H*W, C]; kernel None: global"""
    B, N, C = x.shape
    qkv = x.reshape(B * N, C) @ sd[pre + "qkv.weight"].t()
    a = dense_attention(qkv, B, N, heads) if kernel is None else nbr2d_attention(qkv, B, H, W, heads, kernel)
    return _linear(sd, pre + "proj", a).view(B, N, C)


def mixing_block(sd, x, H, W, heads, kernel):
    """MixingBlock on x [B, H*W, C]"""
    x = x + mha(sd, _norm(sd, "norm1", x), H, W, heads, kernel, pre="attn.")
    return x + _linear(sd, "mlp.2", F.gelu(_linear(sd, "mlp.0", _norm(sd, "norm2", x))))


def merging(sd, x, H, W):
    """Merging on x [B, H*W, C] -> [B, Ho*W, out]"""
    B, _, C = x.shape
    z = F.conv2d(x.view(B, H, W, C).permute(0, 3, 1, 2), sd["conv.weight"], sd["conv.bias"], stride=(2, 1), padding=1)
    return _norm(sd, "norm", z.flatten(2).transpose(1, 2))


def run_stage(kind, args, sd, x, H, W):
    """one module of a svtr_cases case -> (y, H, W)"""
    if kind == "block":
        return mixing_block(sd, x, H, W, args[1], (7, 11) if args[2] else None), H, W
    if kind == "attn":
        return mha(sd, x, H, W, args[1], tuple(args[3]) if args[2] else None), H, W
    if kind == "merge":
        return merging(sd, x, H, W), (H - 1) // 2 + 1, W
    if kind == "comb":
        return combining(sd, x, H, W), 1, W
    raise ValueError(kind)


def run_case(stages, x, H, W):
    """stages: [(tag, kind, args, state_dict)] -> the output of the chain"""
    for _, kind, args, sd in stages:
        x, H, W = run_stage(kind, args, sd, x, H, W)
    return x


def case_grads(stages, x, dy, H, W):
    """(y, dx, {tag.name: gradient}) of sum(run_case(..) * dy), float64"""
    leaves = [(tag, kind, args, {k: v.double().clone().requires_grad_(True) for k, v in sd.items()})
              for tag, kind, args, sd in stages]
    xr = x.double().clone().requires_grad_(True)
    y = run_case(leaves, xr, H, W)
    (y * dy.double()).sum().backward()
    grads = {f"{tag}.{k}": v.grad for tag, _, _, sd in leaves for k, v in sd.items()}
    return y.detach(), xr.grad, grads
