"""Host-side restatements for the attention-dropout tests: the counter-based mask of csrc/dropout_common.h in numpy uint64
arithmetic, and float64 torch attention with that mask whose gradients come from autograd.

    keep(b, head, q, k) = keep_elem(seed, ((b h + head) N + q) N + k, thr),   thr = (unsigned)(p 2^24 + 0.5)
    keep_elem(seed, i, thr) = (mix64(seed + G (i + 1)) >> 40) >= thr          (mix64: the splitmix64 finaliser)"""
import math

import numpy as np
import torch

G = np.uint64(0x9E3779B97F4A7C15)
C1 = np.uint64(0xBF58476D1CE4E5B9)
C2 = np.uint64(0x94D049BB133111EB)


def mix64(z):
    """z: uint64 array (the products wrap modulo 2^64)"""
    z = (z ^ (z >> np.uint64(30))) * C1
    z = (z ^ (z >> np.uint64(27))) * C2
    return z ^ (z >> np.uint64(31))


def thr_of(p):
    return int(p * 16777216.0 + 0.5)


def scale_of(p):
    """the float32 factor the kernels multiply kept values by"""
    return float(np.float32(1.0 / (1.0 - p)))


def keep_elems(seed, idx, p):
    """bool array like idx (any integer array of element indices)"""
    idx = np.asarray(idx).astype(np.uint64)
    z = np.full(idx.shape, int(seed) & (2 ** 64 - 1), dtype=np.uint64) + G * (idx + np.uint64(1))
    return (mix64(z) >> np.uint64(40)) >= np.uint64(thr_of(p))


def keep_mask(seed, B, h, N, p):
    """bool [B, h, N, N]: element ((b h + head) N + q) N + k of a dense [B h, N, N] tensor"""
    return keep_elems(seed, np.arange(B * h * N * N, dtype=np.uint64), p).reshape(B, h, N, N)


def attention_ref(qkv, B, N, h, hd, keep=None, p=0.0, bias=None, dout=None):
    """float64 softmax(q k^T hd^-0.5 + bias) * keep / (1 - p) @ v over the [B, N, 3, h, hd] layout.
    qkv: [B*N, 3*h*hd] (any dtype, taken as given); keep: bool [B, h, N, N] or None; bias: float64 [h, N, N] or None, may
    require grad.  -> (out [B*N, h*hd], lse2 [B, h, N] of the undropped softmax, dqkv or None); with dout the backward has
    run, so a bias that requires grad holds its gradient."""
    x = qkv.double().reshape(B, N, 3, h, hd).permute(2, 0, 3, 1, 4).clone().requires_grad_(dout is not None)
    q, k, v = x[0], x[1], x[2]
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    if bias is not None:
        s = s + bias.unsqueeze(0)
    pr = s.softmax(-1)
    if keep is not None:
        pr = pr * torch.as_tensor(keep).double() / (1.0 - p)
    o = (pr @ v).permute(0, 2, 1, 3).reshape(B * N, h * hd)
    lse2 = (torch.logsumexp(s, -1) * math.log2(math.e)).detach()
    if dout is None:
        return o.detach(), lse2, None
    o.backward(dout.double())
    return o.detach(), lse2, x.grad.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * h * hd)


def table_bias(table, N, P, ws, shift):
    """dense float64 [h, N, N] score bias of the window fork from its table [(2P-1), h] (differentiable in the table):
    the entry variants.relative_position_index names inside a window, -inf outside"""
    from htrvt_amd import variants as V
    idx, inside = V.relative_position_index(N, P, ws, shift)
    bias = table.double()[idx].permute(2, 0, 1)
    return bias.masked_fill(~inside.unsqueeze(0), float("-inf"))
