"""Plain-torch float64 statements of csrc/swin.hip's attention in the kernel's own layout (token-order qkv, index arithmetic
for roll / partition / reverse, the bias table, the two-region additive mask) and of the three module sequences of
htr-vt_amd/swin.py.  tests/test_swin_cpu.py anchors them to the fork's own float64 results (tests/golden/swin.npz); the GPU
tests compare the kernels and modules with them.  Everything is differentiable by autograd."""
import torch
import torch.nn.functional as F


def window_slots(H, W, window, shift):
    """(tok [nWin, n] int64: the token h * W + w that slot t of window (i, j) reads and writes, reg [nWin, n]: its region)"""
    (wh, ww), (sh, sw) = window, shift
    i, j = torch.arange(H // wh), torch.arange(W // ww)
    r, c = torch.arange(wh), torch.arange(ww)
    hs = (i[:, None, None, None] * wh + r[None, None, :, None]).expand(H // wh, W // ww, wh, ww)
    ws = (j[None, :, None, None] * ww + c[None, None, None, :]).expand(H // wh, W // ww, wh, ww)
    tok = ((hs + sh) % H) * W + (ws + sw) % W
    reg = ((hs >= H - sh) & (sh > 0)).long() + 2 * ((ws >= W - sw) & (sw > 0)).long()
    return tok.reshape(-1, wh * ww), reg.reshape(-1, wh * ww)


def table_index(window):
    """idx [n, n]: the table entry of (query t, key u)"""
    wh, ww = window
    t = torch.arange(wh * ww)
    r, c = t // ww, t % ww
    return (r[:, None] - r[None, :] + wh - 1) * (2 * ww - 1) + (c[:, None] - c[None, :] + ww - 1)


def win2d_scores(qkv, table, B, H, W, heads, window, shift, masked=True, mask_value=-100.0):
    """(S [B, nWin, heads, n, n] pre-softmax, v [B, nWin, heads, n, hd], tok)"""
    D = qkv.shape[1] // 3
    hd = D // heads
    tok, reg = window_slots(H, W, window, shift)
    g = qkv.view(B, H * W, 3, heads, hd)[:, tok]                      # [B, nWin, n, 3, heads, hd]
    q, k, v = [g[:, :, :, a].permute(0, 1, 3, 2, 4) for a in range(3)]
    S = (q @ k.transpose(-1, -2)) * hd ** -0.5 + table[table_index(window)].permute(2, 0, 1).to(qkv.dtype)
    if masked:
        differ = reg[:, :, None] != reg[:, None, :]
        S = S + torch.where(differ, mask_value, 0.0).to(qkv.dtype)[None, :, None]
    return S, v, tok


def win2d_attention(qkv, table, B, H, W, heads, window, shift, masked=True, mask_value=-100.0):
    """qkv [B*H*W, 3*heads*hd] -> out [B*H*W, heads*hd]"""
    S, v, tok = win2d_scores(qkv, table, B, H, W, heads, window, shift, masked, mask_value)
    o = (S.softmax(-1) @ v).permute(0, 1, 3, 2, 4).reshape(B, H * W, -1)   # rows in slot order (window, t)
    return o[:, torch.argsort(tok.reshape(-1))].reshape(B * H * W, -1)


def win2d_grads(qkv, table, dout, B, H, W, heads, window, shift):
    """(out, dqkv, dtable) of sum(out * dout)"""
    qr, tr = qkv.clone().requires_grad_(True), table.to(qkv.dtype).clone().requires_grad_(True)
    out = win2d_attention(qr, tr, B, H, W, heads, window, shift)
    (out * dout).sum().backward()
    return out.detach(), qr.grad, tr.grad


def pinned_mask_case(dtype=torch.float64):
    """(1,1,8,1,32,1,8,0,4): q = 32 e0 for slots of the first region, k = 32 e0 for slots of the second, v = the slot's
    number in every element, everything else zero -- exact in bfloat16.  The masked raw score is 1024 / sqrt(32) = 181"""
    tok, reg = window_slots(1, 8, (1, 8), (0, 4))
    qkv = torch.zeros(8, 3, 32, dtype=dtype)
    qkv[tok[0][reg[0] == 0], 0, 0] = 32.0
    qkv[tok[0][reg[0] != 0], 1, 0] = 32.0
    qkv[tok[0], 2, :] = torch.arange(8, dtype=dtype)[:, None]
    return qkv.view(8, 96), torch.zeros(15, 1, dtype=dtype)


def _linear(sd, name, x):
    return x @ sd[name + ".weight"].t() + sd[name + ".bias"]


def _norm(sd, name, x):
    return F.layer_norm(x, x.shape[-1:], sd[name + ".weight"], sd[name + ".bias"], 1e-5)


def window_attention(sd, x, heads, window):
    """WindowAttention2D on partitioned windows x [Bn, wh*ww, C], no mask"""
    Bn, n, C = x.shape
    a = win2d_attention(_linear(sd, "qkv", x.reshape(Bn * n, C)), sd["relative_position_bias_table"], Bn, window[0], window[1],
                        heads, window, (0, 0))
    return _linear(sd, "proj", a).view(Bn, n, C)


def swin_block(sd, x, H, W, heads, window, shift):
    """SwinBlock2D on x [B, H*W, C]"""
    B, N, C = x.shape
    qkv = _linear(sd, "attn.qkv", _norm(sd, "norm1", x).reshape(B * N, C))
    a = win2d_attention(qkv, sd["attn.relative_position_bias_table"], B, H, W, heads, window, shift)
    x = x + _linear(sd, "attn.proj", a).view(B, N, C)
    return x + _linear(sd, "mlp.3", F.gelu(_linear(sd, "mlp.0", _norm(sd, "norm2", x))))


def patch_merge(sd, x, H, W):
    """HeightOnlyPatchMerging on x [B, H*W, C] -> [B, (H/2)*W, out]"""
    B, _, C = x.shape
    w = sd["reduce.weight"]
    x5 = x.view(B, H // 2, 2, W, C)
    z = x5[:, :, 0] @ w[:, :, 0, 0].t() + x5[:, :, 1] @ w[:, :, 1, 0].t()
    return _norm(sd, "norm", z.reshape(B, H // 2 * W, -1))


def combining(sd, x, H, W):
    """Combining on x [B, H*W, C] -> [B, W, out]"""
    B, _, C = x.shape
    return F.gelu(_linear(sd, "fc", x.view(B, H, W, C).mean(1)))


def run_stage(kind, args, sd, x, H, W):
    """one module of a swin_cases case -> (y, H, W)"""
    if kind == "block":
        return swin_block(sd, x, H, W, args[1], args[2], args[3]), H, W
    if kind == "merge":
        return patch_merge(sd, x, H, W), H // 2, W
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
    leaves = [(tag, kind, args, {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v)
                                 for k, v in sd.items()}) for tag, kind, args, sd in stages]
    xr = x.double().clone().requires_grad_(True)
    y = run_case(leaves, xr, H, W)
    (y * dy.double()).sum().backward()
    grads = {f"{tag}.{k}": v.grad for tag, _, _, sd in leaves for k, v in sd.items() if v.is_floating_point()}
    return y.detach(), xr.grad, grads
