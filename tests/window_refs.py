"""Host-side references for the per-element tests of the window and neighbourhood attention kernels that keep their scores
on the VALU (csrc/window_attn_impl.h: lgp.hip's 1-D windows, swin.hip's 2-D windows, svtr.hip's clipped boxes):
tests/test_window_refs_cpu.py proves what is claimed here on the host, tests/test_window_edges_gpu.py holds the kernels to it.

All three operations are dense attention over a short token list with a structured additive score term, so each geometry is
turned into the dense form of attn_refs.attention_f64 (`form_local`, `form_win2d`, `form_nbr2d` -> `reference`):
  1-D local    N + pad tokens per image, the pad rows equal to qkv_bias; token j sits in slot (j + shift) mod N, the pad rows in
               slots N ..., window = slot // w; 0 inside a window, -inf outside.  dpad [B][2D] = the k and v gradient of the pad
               rows, summed over them
  2-D windows  H W tokens in place; slot (r, c) of window (i, j) is token ((i wh + r + sh) mod H, (j ww + c + sw) mod W); table
               entry of the pair, -100 where the regions of the two slots differ, -inf between windows.  dtable[e][head] = the sum
               of dscore over the pairs that use entry e
  box          H W tokens; 0 where |y - y'| <= kh / 2 and |x - x'| <= kw / 2, -inf elsewhere; lse is the natural log-sum-exp

Per-element error model, bfloat16 (u = 2^-8), from the rounding points of the kernels: Axpy2<bf16_t>::coef rounds the pair of
coefficients of every accumulation -- the unnormalised exp(s - m) in the forward (the row sum takes the unrounded values),
scale dS in front of the dq and dk products, P in front of dv --, and out / dq / dk / dv are stored as bfloat16:
    E_O  = u (sum_k P |v| + |O|)            E_dV = u (sum_q P |dO| + |dV|)
    E_dS = u |dS| + scale P E_delta         E_dQ = sum_k E_dS |K| + u |dQ|      E_dK = sum_q E_dS |Q| + u |dK|
    E_dscore = P E_delta + 2^-20 |dscore|   E_dtable[e] = sum of E_dscore over the entry's pairs
    E_dpad   = (pad rows) x the dK / dV bound of a pad row without the storage term (dpad is float32)
The window kernels form delta = sum_j P dP in float32 from recomputed values: E_delta = 0.  The box kernels form it from the
stored bfloat16 out (and P from the stored float32 lse): E_delta = u sum_d |dO| |O|, as in attn_refs.error_model.  Every
bound gets the float32 floor added, 8 E32 max|ref| of its output (kernel_refs.e32: the float32 evaluation error of the reference
on these very inputs), so that an element whose bfloat16 terms vanish is not held to zero; the float32 instances, lse and the
float32 sums of the float32 instances are held to that floor alone (kernel_refs.gate_check's rule, per element).  (Plus FLUSH,
the smallest normal float32, per element: what float64 keeps below it, the kernels flush to zero.)

`emulate_bf16` applies exactly those roundings to float32 scores / exp / sums.  On every random case of the lists below (the
GPU file uses the same lists and seeds) it stays within 1.0 x the model; worst ratios measured on the CPU: EMULATION_WORST,
asserted as a ceiling by the CPU test.  The GPU tests allow attn_refs.C_GPU = 2.0 x the model, under the rule of attn_refs: a
kernel past it is a finding, the constant is never raised.

`ref_local` / `ref_shifted` are the float64 restatements of the forks' WindowMHSA1D that tests/test_lgp_kernels_gpu.py and
tests/test_local_shift_gpu.py use (moved here, not forked).  Constructions with exact expectations: membership_probe,
one_hot_groups (each says why it is exact)."""
import functools
from types import SimpleNamespace

import torch

import attn_refs as A
import kernel_refs as K
from attn_refs import C_GPU, U, assert_guards_intact, bf16, guarded, merge_heads, split_heads, worst_ratio  # noqa: F401

NEG = float("-inf")
F32_FACTOR = 8.0
FLUSH = 2.0 ** -126                   # smallest normal float32 (and bfloat16)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
# worst |emulation - float64| / model over the random cases below, per family and output (asserted as a ceiling, with 1.0)
EMULATION_WORST = {
    "local": {"out": 0.81, "dqkv": 0.92, "dpad": 0.91},
    "win2d": {"out": 0.84, "dqkv": 0.95, "dtable": 0.14},
    "nbr2d": {"out": 0.76, "lse": 0.15, "dqkv": 0.87},
}

# ---- case lists (shared by the CPU and the GPU file) --------------------------------------------------------------------
# 1-D local, (B, N, heads, w, shift); shift None: the plain entry point.  Waves per workgroup of the instances (bfloat16 hd
# 128 / 64, float32 hd 128 / 64): forward 4 / 4 / 2 / 4, backward 2 / 4 / 1 / 2; units = B ceil(N / w) heads.  Every case runs
# at hd 64 and 128 in both dtypes.
LOCAL_CASES = [
    (2, 5, 3, 1, None),       # w = 1: every token alone, 30 units, no padding
    (1, 1, 1, 2, None),       # N = 1 < w: one unit, one token and one padding row
    (3, 7, 2, 2, 1),          # N % w = 1 = w - 1, shift 1: 24 units
    (1, 8, 3, 2, None),       # a multiple of w: dpad exactly zero; 12 units
    (1, 1, 1, 15, None),      # one token, 14 padding rows, odd window
    (1, 14, 1, 15, 13),       # N = w - 1, shift N - 1: the wrap and the padding row in one window, one unit
    (2, 16, 3, 15, 1),        # N % w = 1: 12 units
    (1, 29, 1, 15, 14),       # N % w = w - 1, shift w - 1: 2 units
    (3, 30, 1, 15, None),     # a multiple of w, odd window: 6 units
    (1, 1, 1, 16, None),      # one token, 15 padding rows
    (1, 15, 3, 16, 14),       # N = w - 1, shift N - 1: 3 units
    (2, 17, 1, 16, 15),       # N % w = 1, shift w - 1: 4 units
    (1, 31, 1, 16, 1),        # N % w = w - 1, shift 1: 2 units
    (1, 32, 1, 16, 8),        # a multiple of w, shifted: dpad exactly zero
    (1, 8, 1, 12, 7),         # the forks' 12: N < w, shift N - 1
    (2, 20, 3, 12, 11),       # N % w = 8, shift w - 1: 12 units
    (3, 25, 2, 12, 1),        # N % w = 1: 18 units
    (1, 23, 1, 12, 6),        # N % w = w - 1: 2 units
    (1, 24, 2, 12, 6),        # a multiple of w, shifted
    (1, 100, 1, 12, None),    # 9 units: not a multiple of 2 or 4
]
LOCAL_HD = (64, 128)
# 2-D windows, (B, H, W, heads, hd, wh, ww, sh, sw).  Waves per workgroup (bfloat16 hd 128 / 64 / 32, float32 the same):
# 2 / 2 / 4 and 1 / 2 / 2, forward and backward; the backward walks items = B (H / wh)(W / ww) in min(items, 256) shares
WIN2D_CASES = [
    (1, 4, 8, 1, 32, 4, 8, 3, 7),         # 32 tokens 4 x 8, both shifts at their extreme, H == wh with sh > 0, one item
    (2, 2, 32, 6, 64, 2, 16, 1, 15),      # 2 x 16, 6 heads, 4 items
    (1, 2, 32, 1, 128, 1, 32, 0, 31),     # 1 x 32, (0, sw), 2 items
    (2, 6, 10, 1, 64, 3, 5, 2, 0),        # odd 15 tokens, (sh, 0), 8 items
    (1, 3, 9, 6, 32, 3, 3, 2, 2),         # odd 9 tokens, H == wh with sh > 0, 3 items (fewer than the waves), 6 heads
    (1, 5, 10, 1, 128, 5, 5, 4, 4),       # odd 25 tokens, 2 items
    (3, 8, 16, 1, 32, 4, 8, 2, 4),        # 12 items in workgroups of 4 and 2 waves
    (2, 3, 5, 1, 32, 1, 1, 0, 0),         # 1 x 1: out = v, dq = dk = 0; 30 items
    (1, 16, 32, 1, 64, 1, 2, 0, 1),       # 256 items: exactly the most partial rows
    (1, 10, 60, 1, 32, 1, 2, 0, 1),       # 300 items in 256 shares of 1 or 2: waves past a share's end run the zero rows
    (1, 9, 58, 2, 128, 1, 2, 0, 1),       # 261 items, one wave per workgroup in float32
]
# boxes, (B, H, W, heads, hd, kh, kw).  Query tiles of TH x 16; TH = 8 only for bfloat16 hd 32 where ceil(H / 8) 8 <= ceil(H / 4) 4
NBR2D_CASES = [
    (1, 1, 1, 1, 32, 7, 11),              # one token: the map is smaller than half the box both ways
    (3, 2, 3, 2, 32, 7, 11),              # the same, several images and heads
    (2, 4, 15, 2, 32, 7, 11),
    (1, 5, 16, 1, 64, 3, 5),
    (1, 5, 17, 2, 32, 3, 5),
    (1, 8, 17, 2, 32, 7, 1),
    (1, 9, 33, 1, 32, 1, 11),
    (1, 12, 1, 3, 64, 7, 11),             # W = 1
    (1, 12, 15, 1, 32, 3, 5),
    (1, 16, 17, 1, 32, 7, 11),            # two tile rows of 8 (bfloat16), four of 4 (float32); two tile columns
    (1, 16, 33, 1, 64, 3, 5),
    (2, 8, 16, 1, 64, 7, 11),
    (1, 4, 33, 2, 64, 1, 11),
    (2, 9, 15, 1, 64, 7, 1),
    (40, 3, 5, 1, 32, 3, 5),              # many images with a map smaller than one tile
    (2, 5, 15, 1, 32, 1, 1),              # self only: out = v
    (1, 8, 16, 2, 64, 1, 1),
]
LOCAL_FULL = [(B, N, h, hd, w, shift) for B, N, h, w, shift in LOCAL_CASES for hd in LOCAL_HD]    # form_local's arguments
FAMILIES = {"local": LOCAL_FULL, "win2d": WIN2D_CASES, "nbr2d": NBR2D_CASES}


def nbr2d_tile_rows(hd, dtype, H):
    """rows of the query tile include/htrvt.h promises: 8 for bfloat16 hd 32 where 8-row tiles leave no more idle rows"""
    return 8 if (dtype == BF and hd == 32 and (H + 7) // 8 * 8 <= (H + 3) // 4 * 4) else 4


def local_units(B, N, h, w):
    return B * ((N + w - 1) // w) * h


# ---- the forks' 1-D window attention, restated (moved from the two GPU test files) --------------------------------------
def ref_local(qkv, bias, B, N, h, hd, w):
    """WindowMHSA1D.forward (plg.py:109-137) on the qkv Linear's output: a zero padding token leaves the Linear as its bias"""
    D = h * hd
    x = qkv.reshape(B, N, 3 * D)
    pad = (w - N % w) % w
    if pad:
        x = torch.cat([x, bias.reshape(1, 1, 3 * D).expand(B, pad, 3 * D)], dim=1)
    Np = N + pad
    q, k, v = x.reshape(B * (Np // w), w, 3, h, hd).permute(2, 0, 3, 1, 4).unbind(0)
    a = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
    out = (a @ v).transpose(1, 2).reshape(B, Np, D)
    return out[:, :N].reshape(B * N, D)


def ref_shifted(qkv, bias, B, N, h, hd, w, s, mask_wrap=False):
    """[B*N, 3D] float64 -> [B*N, D]; mask_wrap: the Swin-style mask the fork does NOT have (no attention between the tokens
    rolled in from the end of the line and the ones from its start)"""
    D = h * hd
    x = qkv.reshape(B, N, 3 * D)
    s = s % w
    if s:
        x = torch.roll(x, shifts=s, dims=1)
    pad = (w - N % w) % w
    if pad:
        x = torch.cat([x, bias.reshape(1, 1, 3 * D).expand(B, pad, 3 * D)], dim=1)
    Np = N + pad
    nW = Np // w
    q, k, v = x.reshape(B * nW, w, 3, h, hd).permute(2, 0, 3, 1, 4).unbind(0)
    sc = (q @ k.transpose(-2, -1)) * hd ** -0.5                      # [B nW, h, w, w]
    if mask_wrap:
        side = (torch.arange(Np) < (s % N)).reshape(nW, w)            # slots holding tokens from the end of the line
        cross = (side[:, :, None] != side[:, None, :]).repeat(B, 1, 1)[:, None]
        sc = sc.masked_fill(cross, float("-inf"))
    out = (sc.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, Np, D)[:, :N]
    if s:
        out = torch.roll(out, shifts=-s, dims=1)
    return out.reshape(B * N, D)


# ---- geometry -> dense form ---------------------------------------------------------------------------------------------
def form_local(B, N, h, hd, w, shift, slot_token=None):
    """tokens 0 .. N - 1, then the pad rows.  slot_token: {slot: token} overrides of which token a slot reads (a fault to
    inject); a token that several slots of a window read counts that often (`count`), one that none reads does not exist"""
    s = (shift or 0) % N
    pad = (w - N % w) % w
    Nd = N + pad
    token_of_slot = torch.cat([(torch.arange(N) - s) % N, torch.arange(N, Nd)])      # Local1d::unit
    for p, t in (slot_token or {}).items():
        token_of_slot[p] = t
    win_of_slot = torch.arange(Nd) // w
    win_of_token = torch.empty(Nd, dtype=torch.long)
    win_of_token[torch.cat([(torch.arange(N) - s) % N, torch.arange(N, Nd)])] = win_of_slot       # where a token's query sits
    count = torch.zeros(Nd, Nd)                             # [query token, key token]
    for p in range(Nd):
        count[win_of_token == win_of_slot[p], token_of_slot[p]] += 1
    return SimpleNamespace(kind="local", B=B, N=N, Nd=Nd, pad=pad, h=h, hd=hd, w=w, shift=s, count=count, inside=count > 0,
                           win_of_token=win_of_token)


def form_win2d(B, H, W, h, hd, wh, ww, sh, sw):
    N, n = H * W, wh * ww
    t = torch.arange(N)
    ty, tx = t // W, t % W
    hs, ws = (ty - sh) % H, (tx - sw) % W                   # the slot's place in the rolled map: token = (hs + sh, ws + sw)
    win = (hs // wh) * (W // ww) + ws // ww
    r, c = hs % wh, ws % ww
    reg = ((hs >= H - sh) & (sh > 0)).long() + 2 * ((ws >= W - sw) & (sw > 0)).long()
    inside = win[:, None] == win[None, :]
    idx = (r[:, None] - r[None, :] + wh - 1) * (2 * ww - 1) + (c[:, None] - c[None, :] + ww - 1)
    return SimpleNamespace(kind="win2d", B=B, N=N, Nd=N, pad=0, h=h, hd=hd, H=H, W=W, window=(wh, ww), shift=(sh, sw), n=n,
                           inside=inside, idx=idx, differ=reg[:, None] != reg[None, :], win=win, slot=r * ww + c, reg=reg,
                           TE=(2 * wh - 1) * (2 * ww - 1), items=B * (H // wh) * (W // ww))


def form_nbr2d(B, H, W, h, hd, kh, kw):
    N = H * W
    t = torch.arange(N)
    y, x = t // W, t % W
    inside = ((y[:, None] - y[None, :]).abs() <= kh // 2) & ((x[:, None] - x[None, :]).abs() <= kw // 2)
    return SimpleNamespace(kind="nbr2d", B=B, N=N, Nd=N, pad=0, h=h, hd=hd, H=H, W=W, box=(kh, kw), inside=inside)


def make_form(family, case):
    if family == "local":
        B, N, h, hd, w, shift = case
        return form_local(B, N, h, hd, w, shift)
    if family == "win2d":
        return form_win2d(*case)
    return form_nbr2d(*case)


def dense_bias(form, side, dtype=F64, mask_value=-100.0):
    """[h, Nd, Nd] additive score term; side: the table [TE, h] of a 2-D window (else unused)"""
    if form.kind == "win2d":
        b = side.to(dtype)[form.idx].permute(2, 0, 1) + torch.where(form.differ, mask_value, 0.0).to(dtype)
        return torch.where(form.inside, b, torch.full_like(b, NEG))
    if form.kind == "local":
        b = torch.log(form.count).to(dtype)                 # 0 inside a window, -inf outside (log 2 for a doubled key)
    else:
        b = torch.where(form.inside, 0.0, NEG).to(dtype)
    return b.unsqueeze(0).expand(form.h, form.Nd, form.Nd)


def _dense_operands(form, qkv, side, dout, dtype):
    B, N, D = form.B, form.N, form.h * form.hd
    x = qkv.to(dtype).reshape(B, N, 3 * D)
    g = None if dout is None else dout.to(dtype).reshape(B, N, D)
    if form.pad:
        x = torch.cat([x, side.to(dtype).reshape(1, 1, 3 * D).expand(B, form.pad, 3 * D)], dim=1)
        if g is not None:
            g = torch.cat([g, torch.zeros(B, form.pad, D, dtype=dtype)], dim=1)     # a padded query's output is cropped
    return x.reshape(B * form.Nd, 3 * D), None if g is None else g.reshape(B * form.Nd, D)


def scatter_entries(form, x):
    """[B, h, N, N] per-pair values -> [TE, h]: the sum over the images and the pairs that use each table entry"""
    xs = x.sum(0)
    out = torch.zeros(form.TE, form.h, dtype=x.dtype)
    for hh in range(form.h):
        out[:, hh].index_add_(0, form.idx[form.inside], xs[hh][form.inside])
    return out


def collect(form, r, raw=False):
    """the kernel-layout outputs of a dense result: out [B*N, D], lse [B*h, N], dqkv [B*N, 3D], dpad [B, 2D] (local),
    dtable [TE, h] (win2d).  raw: dpad from r.dK_raw / r.dV_raw (gradients before their storage rounding)"""
    B, N, Nd, D = form.B, form.N, form.Nd, form.h * form.hd

    def crop(x):
        return x.reshape(B, Nd, -1)[:, :N].reshape(B * N, -1)

    o = SimpleNamespace(out=crop(r.O), lse=r.lse[:, :, :N].reshape(B * form.h, N))
    if not hasattr(r, "dQ"):
        return o
    o.dqkv = torch.cat([crop(r.dQ), crop(r.dK), crop(r.dV)], dim=1)
    if form.kind == "local":
        dk, dv = (r.dK_raw, r.dV_raw) if raw else (r.dK, r.dV)
        o.dpad = torch.cat([dk.reshape(B, Nd, D)[:, N:].sum(1), dv.reshape(B, Nd, D)[:, N:].sum(1)], dim=1)
    if form.kind == "win2d":
        o.dtable = scatter_entries(form, r.dscore)
    return o


def reference(form, qkv, side, dout=None, dtype=F64, bias=None):
    """(dense attention_f64 result, its outputs in the kernels' layouts), evaluated in `dtype`"""
    x, g = _dense_operands(form, qkv, side, dout, dtype)
    r = A.attention_f64(x, form.B, form.Nd, form.h, form.hd, bias=dense_bias(form, side, dtype) if bias is None else bias,
                        dout=g, dtype=dtype, delta_from_p=form.kind != "nbr2d")
    return r, collect(form, r)


OUTPUTS = {"local": ("out", "dqkv", "dpad"), "win2d": ("out", "dqkv", "dtable"), "nbr2d": ("out", "lse", "dqkv")}


def float32_floor(form, qkv, side, dout):
    """{output: 8 E32 max|ref|}: kernel_refs.e32 of the dense reference on these very inputs"""
    names = OUTPUTS[form.kind]

    def fn(q, s, g):
        o = reference(form, q, s, g, dtype=q.dtype)[1]
        return tuple(getattr(o, n) for n in names)

    ref, errs = K.e32(fn, (qkv.float(), None if side is None else side.float(), dout.float()))
    return {n: F32_FACTOR * e * float(x.abs().max()) for n, x, e in zip(names, ref, errs)}


def error_model(form, r):
    """{output: per-element bound} of the bfloat16 kernels (module docstring), without the float32 floor"""
    P, Pt = r.P, r.P.transpose(-1, -2)
    E = SimpleNamespace(lse=torch.zeros_like(r.lse))
    E.O = U * (merge_heads(P @ r.v.abs()) + r.O.abs())
    E.dV_raw = U * merge_heads(Pt @ r.do.abs())
    E.dV = E.dV_raw + U * r.dV.abs()
    e_delta = U * (r.do.abs() * r.o.abs()).sum(-1) if form.kind == "nbr2d" else torch.zeros_like(r.delta)
    pe = P * e_delta.unsqueeze(-1)
    E.dscore = pe + 2.0 ** -20 * r.dscore.abs()
    e_ds = U * r.scale * r.dscore.abs() + r.scale * pe
    E.dQ = merge_heads(e_ds @ r.k.abs()) + U * r.dQ.abs()
    E.dK_raw = merge_heads(e_ds.transpose(-1, -2) @ r.q.abs())
    E.dK = E.dK_raw + U * r.dK.abs()
    return vars(collect(form, E, raw=True))


def bounds(form, r, floor, dtype):
    """{output: per-element bound}: the float32 floor, for bfloat16 behind the model.  Where an output's reference is
    zero throughout the floor is zero and the output must be exactly zero; elsewhere every element is allowed FLUSH, the
    smallest normal float32: below it the kernels' exp and their bfloat16 / float32 stores give 0 where float64 keeps a
    number (a pair across the -100 mask weighs exp(-100) = 4e-44)"""
    o = vars(collect(form, r))
    E = error_model(form, r) if dtype == BF else {}
    out = {}
    for n in OUTPUTS[form.kind]:
        b = torch.full_like(o[n], floor[n] + (FLUSH if float(o[n].abs().max()) > 0 else 0.0))
        out[n] = b + E[n] if dtype == BF and n != "lse" else b
    return out


def limit(dtype):
    """what a worst ratio may reach on the device: C_GPU x the model in bfloat16, the float32 rule itself in float32"""
    return C_GPU if dtype == BF else 1.0


def emulate_bf16(form, qkv, side, dout):
    """the dense attention with the roundings of the bfloat16 kernels and nothing else: float32 scores, exp, row sum, lse,
    dP, delta and dS; exp(s - m) rounded to bfloat16 in front of P v (the row sum takes the unrounded values), scale dS in
    front of the dq and dk products, P in front of dv, bfloat16 out / dq / dk / dv.  delta: sum_j P dP from the recomputed
    row (windows), or dO . out from the stored out with P = exp(s - lse) (boxes).  The products themselves are summed in
    float64.  -> the outputs in the kernels' layouts (dpad from the gradients before their storage rounding)"""
    B, Nd, h, hd = form.B, form.Nd, form.h, form.hd
    x, g = _dense_operands(form, qkv, side, dout, F64)
    q, k, v = split_heads(x, B, Nd, h, hd)
    scale = torch.tensor(hd ** -0.5, dtype=F32)
    s = (q @ k.transpose(-1, -2)).float() * scale + dense_bias(form, side, F32).unsqueeze(0)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    o = bf16((bf16(p) @ v) / l.double())
    r = SimpleNamespace(O=merge_heads(o), lse=lse.squeeze(-1).double())
    do = split_heads(g, B, Nd, h, hd, parts=1)[0]
    dP = (do @ v.transpose(-1, -2)).float()
    if form.kind == "nbr2d":
        P = torch.exp(s - lse)
        delta = (do.float() * o.float()).sum(-1)
    else:
        P = p * (1.0 / l)
        delta = (P * dP).sum(-1)
    dscore = P * (dP - delta.unsqueeze(-1))
    dS, Pb = bf16(dscore * scale), bf16(P)
    r.dscore = dscore.double()
    r.dK_raw, r.dV_raw = merge_heads(dS.transpose(-1, -2) @ q), merge_heads(Pb.transpose(-1, -2) @ do)
    r.dQ, r.dK, r.dV = bf16(merge_heads(dS @ k)), bf16(r.dK_raw), bf16(r.dV_raw)
    return collect(form, r, raw=True)


# ---- random inputs and the cases' references, computed once per process ---------------------------------------------
def random_inputs(family, case, dtype):
    """(qkv, side, dout) already rounded to dtype (side: the 1-D kernels' qkv_bias, rounded too, so that the padding rows are
    the same numbers on both sides; the float32 table of the 2-D windows, entries of order 1; None for the boxes)"""
    form = make_form(family, case)
    g = torch.Generator().manual_seed(1000 * (1 + list(FAMILIES).index(family)) + FAMILIES[family].index(case))
    D = form.h * form.hd
    qkv = torch.randn(form.B * form.N, 3 * D, generator=g).to(dtype)
    dout = torch.randn(form.B * form.N, D, generator=g).to(dtype)
    side = None
    if family == "local":
        side = torch.randn(3 * D, generator=g).to(dtype).float()
    elif family == "win2d":
        side = torch.randn(form.TE, form.h, generator=g)
    return qkv, side, dout


@functools.lru_cache(maxsize=None)
def case_reference(family, case, dtype):
    """namespace: form, qkv / side / dout, r (dense float64 result), ref (its outputs, kernel layouts), bound {output: tensor}"""
    form = make_form(family, case)
    qkv, side, dout = random_inputs(family, case, dtype)
    r, ref = reference(form, qkv, side, dout)
    floor = float32_floor(form, qkv, side, dout)
    return SimpleNamespace(form=form, qkv=qkv, side=side, dout=dout, r=r, ref=vars(ref), floor=floor,
                           bound=bounds(form, r, floor, dtype))


# ---- constructions with exact expectations ----------------------------------------------------------------------------
def ulp(x, dtype):
    """spacing of `dtype` at |x| (float64 tensor of positive values)"""
    bits = 7 if dtype == BF else 23
    return torch.exp2(torch.floor(torch.log2(x)) - bits)


def membership_probe(form, t0, channel, dtype, image=0, head=0):
    """q = 0 (and a zero table / zero qkv_bias): every score of a query is 0 over its key set, so P = 1 / n(query) there --
    except across the mask regions of a shifted 2-D window, whose -100 leaves exp(-100) < 1e-43.  v is the indicator of token
    t0 of one image and head in one channel.  Then out[query] = 1 / n(query) where t0 is one of the query's keys (the unrounded
    coefficient is exactly 1 and the accumulation exactly 1, so only the division and the storage round: 2 ulp), below 1e-40
    where t0 is in the query's window but across the mask, and exactly 0 everywhere else: the key set of every query,
    independently of rounding.  n counts the padding rows of a 1-D window (they are attended) and, in 2-D, the slots of the
    query's own region.  lse of a box is log n.
    -> namespace qkv, side, n [N] (float64), member [N] bool (t0 is a key of the query), masked [N] bool"""
    B, N, h, hd = form.B, form.N, form.h, form.hd
    D = h * hd
    qkv = torch.zeros(B, N, 3, h, hd)
    qkv[image, t0, 2, head, channel] = 1.0
    side = None
    if form.kind == "local":
        side = torch.zeros(3 * D)
    if form.kind == "win2d":
        side = torch.zeros(form.TE, h)
    keys = form.inside[:N, :]
    masked = torch.zeros(N, dtype=torch.bool)
    if form.kind == "win2d":
        masked = keys[:, t0] & form.differ[:, t0]
        keys = keys & ~form.differ
    return SimpleNamespace(qkv=qkv.reshape(B * N, 3 * D).to(dtype), side=side, n=keys.sum(-1).double(),
                           member=keys[:, t0].clone(), masked=masked)


def key_groups(form):
    """the token sets inside which a one-hot permutation may match: the tokens of a 1-D window, the slots of one region of a
    2-D window (a match across the mask would stand only 81 above the rest, not far enough to flush), column pairs of a box
    map (every box that is wider than one column holds its query's neighbour)"""
    N = form.N
    if form.kind == "local":
        key = form.win_of_token[:N]
    elif form.kind == "win2d":
        key = form.win * 4 + form.reg
    else:
        x = torch.arange(N) % form.W
        key = (torch.arange(N) // form.W) * form.W + (x // 2 if form.box[1] >= 3 else x)
    return [torch.nonzero(key == u).flatten() for u in key.unique()]


def code_ids(form):
    """a code number per token that differs between any two keys of one query: the slot of a window, the residue of a box"""
    N = form.N
    if form.kind == "local":
        return ((torch.arange(N) + form.shift) % N) % form.w
    if form.kind == "win2d":
        return form.slot
    kh, kw = form.box
    t = torch.arange(N)
    return ((t // form.W) % kh) * kw + (t % form.W) % kw


def one_hot_groups(form, seed, dtype):
    """attn_refs.one_hot_case inside the key sets of a window or box geometry: query i and key perm[i] (a permutation inside
    each group of key_groups) share a +-8 code word, code words differ between any two keys of one query and lie at least
    hd / 4 apart, v and dout are integers in [-8, 8]; qkv_bias and the table are zero, so a padding key scores 0.  The
    matched pair scores 64 sqrt(hd) >= 362, any other key of the query at least 32 sqrt(hd) >= 181 less (a padding key 362
    less), so every other probability is below e^-181 and flushes to zero in float32: out[i] = v[perm[i]] and
    dV[perm[i]] = dO[i] bit for bit, dq = dk = 0 (the matched pair has dP == delta as integers).
    -> namespace qkv, side, dout (dtype), O, dV (float32, exact)"""
    B, N, h, hd = form.B, form.N, form.h, form.hd
    g = torch.Generator().manual_seed(seed)
    ids = code_ids(form)
    code = A._code_words(int(ids.max()) + 1, hd, g)[ids] * 8.0          # [N, hd]
    groups = key_groups(form)
    qkv = torch.zeros(B, N, 3, h, hd)
    perm = torch.empty(B, h, N, dtype=torch.long)
    for b in range(B):
        for hh in range(h):
            for grp in groups:
                perm[b, hh, grp] = grp[torch.randperm(len(grp), generator=g)]
            qkv[b, :, 0, hh, :] = code[perm[b, hh]]                     # query i carries the word of key perm[i]
            qkv[b, :, 1, hh, :] = code
    qkv[:, :, 2] = torch.randint(-8, 9, (B, N, h, hd), generator=g).float()
    dout = torch.randint(-8, 9, (B, N, h, hd), generator=g).float()
    O, dV = torch.empty(B, N, h, hd), torch.empty(B, N, h, hd)
    for b in range(B):
        for hh in range(h):
            O[b, :, hh] = qkv[b, perm[b, hh], 2, hh]
            dV[b, perm[b, hh], hh] = dout[b, :, hh]
    D = h * hd
    side = torch.zeros(3 * D) if form.kind == "local" else torch.zeros(form.TE, h) if form.kind == "win2d" else None
    return SimpleNamespace(qkv=qkv.reshape(B * N, 3 * D).to(dtype), side=side, dout=dout.reshape(B * N, D).to(dtype),
                           O=O.reshape(B * N, D), dV=dV.reshape(B * N, D), perm=perm)


# ---- the aggregate gates of the four older GPU files (kept to document what the per-element gate adds) -------------------
OLD_FWD_ABS = {BF: 2.5e-2, F32: 2e-5}
OLD_GRAD_REL = {BF: 3e-2, F32: 1e-4}
OLD_GRAD_COS = {BF: 0.9995, F32: 0.999999}


def old_forward_gate(got, want, dtype):
    return float((got - want).abs().max()) < OLD_FWD_ABS[dtype]


def old_backward_gate(got, want, dtype):
    e = float((got - want).abs().max() / want.abs().max())
    cos = float((got.flatten() @ want.flatten()) / (got.norm() * want.norm()))
    return e <= OLD_GRAD_REL[dtype] and cos > OLD_GRAD_COS[dtype]
