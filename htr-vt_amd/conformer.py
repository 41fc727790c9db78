"""MI355X-native blocks of the convolutional forks (model_sgm_mms_conv/model/HTR_VT.py and
model_sgm_mms_conv_squeeze/model/HTR_VT.py, whose lines 1-168 are identical): the modules their Conformer and SqueezeFormer
encoders are built from.

Drop-ins for
    FeedForward(dim, hidden_dim, dropout=0.1)                lin2(silu(lin1(x)))
    ConvModule(dim, kernel_size=3, dropout=0.1, drop_path=0.0, expansion=1.0)
                                                             x + dropout(pw2(silu(GroupNorm(dwconv(glu(pw1(LN(x))))))))
    ConformerBlock(dim, num_heads, num_patches, ...)         x + 1/2 ffn1 -> + attention -> + conv branch -> + 1/2 ffn2 -> LN
    SqueezeExcite1D(dim, se_ratio=0.25)                      x * sigmoid(fc2(silu(fc1(mean over the tokens))))
    Downsample1D() / Upsample1D()                            avg_pool1d(2, 2) / nearest interpolation along the tokens
    SqueezeConformerBlock(dim, num_heads, num_patches, ...)  the ConformerBlock with the SE gate behind the conv branch
    SqueezeFormerEncoder(dim, num_heads, num_patches, depth, ...)   stage1, down, stage2, up + skip, out_norm
Same module tree, parameter names, shapes (the 1x1 Conv1d weights stay [out, in, 1]) and construction order as the forks',
so `torch.manual_seed(s)` followed by a constructor gives the fork's initial state_dict and a fork checkpoint's entries load
with strict=True.

Every forward is ONE autograd node over the launch sequences of seq_ops: LayerNorm, the GEMMs and their weight gradients,
the attention kernels (plain scores, qkv bias; bfloat16 with N >= 32 the fused kernel, else the unfused GEMM route, the
parity route), and csrc/gnmixer.hip for GLU + depthwise convolution + GroupNorm(1, C) + SiLU, the SE gate, the resampling
and FeedForward's SiLU.  GroupNorm takes the statistics of each image in train and eval mode alike.  Tokens stay [B*N, D]
rows throughout.  Every parameter gradient is float32 and bitwise reproducible.
compute_dtype: torch.float32 (parity) or torch.bfloat16; inputs and outputs are float32.

Train mode runs every regulariser the constructors take, with the forks' semantics: dropout behind the feed-forwards and the
attention's projection (ff_dropout), on the attention probabilities (attn_dropout) and behind the conv branch
(conv_dropout / ConvModule's dropout); four independent DropPath draws per block, one per residual site, by timm's rule
(one Bernoulli(1 - p) per sample, kept samples scaled by 1 / (1 - p)); SqueezeFormerEncoder ramps the blocks' rate up to
drop_path_total.  x + 1/2 drop_path(dropout(lin2(...))) is computed as x + drop_path(dropout(1/2 lin2(...))), and the fork's
x + drop_path(conv_out - x) as x + drop_path(dropout(branch)).  With a regulariser active the GEMM that ends a branch writes
the branch alone and ONE launch of csrc/dropnorm.hip forms the new residual stream and the LayerNorm behind it (backward:
that norm's backward and the branch's masked gradient); behind the SE gate of SqueezeConformerBlock the conv site is
seq_ops.residual_dropout and the plain norm.  With every rate zero, and in eval mode, the launches are those without
regularisers, the adds in the GEMM epilogues.
Masks come from a counter-based generator (csrc/dropout_common.h) keyed by int64 seeds and the element's / sample's index:
nothing is stored, the backward regenerates them.  The seeds are drawn on the device from the CUDA default generator, one
draw per forward of a node and no host sync, distinct per site and per block; `torch.cuda.manual_seed(s)` before two
identical steps gives identical bits.  A module keeps the seeds of its last train-mode forward as `last_drop_seeds` (layout
in the class docstrings), so the masks can be rebuilt outside.
Not served, refused with an error: train mode with a non-zero rate on a tensor that is not on the device (the seeds are drawn
there; the error names the rates); attn_dropout > 0 in train mode where the attention takes the unfused route with a padded
token count (float32 with N off a multiple of 4; bfloat16 with N < 32 off a multiple of 8); hidden widths whose GLU output is
not a multiple of 8; an odd hidden width (the fork's no-GLU path); kernel sizes other than odd 1 ... 15; head widths other
than 32 / 64 / 128.
"""
import torch
import torch.nn as nn

from . import seq_ops
from .swin import _as, _check_device, _check_dtype, _grads, _need, _rows

__all__ = ["FeedForward", "ConvModule", "ConformerBlock", "SqueezeExcite1D", "Downsample1D", "Upsample1D",
           "SqueezeConformerBlock", "SqueezeFormerEncoder"]

HEAD_DIMS = (32, 64, 128)


def _params(names, params, cdt):
    """by name: Linear weights [out, in] and the 1x1 Conv1d weights [out, in, 1] as [out, in] in the compute dtype; the
    excite MLP, the depthwise weight, biases and norms float32 as stored"""
    P = {}
    for n, t in zip(names, params):
        t = t.contiguous()
        if "pointwise_conv" in n and t.dim() == 3:
            t = _as(t.view(t.shape[0], t.shape[1]), cdt)
        elif t.dim() == 2 and "fc1." not in n and "fc2." not in n:
            t = _as(t, cdt)
        P[n] = t
    return P


SITES = ("ffn1", "attn", "conv", "ffn2")          # the residual sites of a block, in the order of its forward
BLOCK_SEEDS = 2 * len(SITES) + 1                  # (element, sample) per site, then the attention probabilities'


def _draw(n, dev):
    """n int64 seeds on the device: one draw from the CUDA default generator, no host sync"""
    return torch.randint(0, 2 ** 62, (n,), dtype=torch.int64, device=dev)


def _rates_need_device(mod, x, **rates):
    """Train mode with a non-zero rate draws the masks' seeds from the CUDA generator of x's device, so a tensor that is not
    on one is refused here, before anything is drawn, and the refusal names the rates that ask for it.  (Eval mode, and train
    mode with every rate zero, draw nothing and reach the generic device check of _apply.)"""
    on = {n: p for n, p in rates.items() if p > 0}
    if mod.training and on and not x.is_cuda:
        raise NotImplementedError(
            f"{type(mod).__name__}: " + ", ".join(f"{n} = {p}" for n, p in on.items()) + " in train mode is served on an MI355X "
            f"only: the masks' seeds are drawn on the device and x is on {x.device} (move the module and its input to cuda, or "
            "call .eval())")


def _site(p, p_path, seeds):
    """a residual site's (p, p_path, seeds) for seq_ops, None when both rates are 0"""
    return (float(p), float(p_path), seeds) if p > 0 or p_path > 0 else None


class _Function(torch.autograd.Function):
    """one node for a whole module: forward(mod, x, need, *params) over mod._fwd / mod._bwd, the seq_ops sequences"""

    @staticmethod
    def forward(ctx, mod, x, need, *params):
        P = _params(mod.PARAMS, params, mod.compute_dtype)
        xr = _rows(x, mod.compute_dtype)
        y, saved, geo, out_shape = mod._fwd(xr, P, x.shape)
        y = _as(y, torch.float32).view(out_shape)
        if need:
            saved = tuple(saved)
            ctx.none = [t is None for t in saved]
            ctx.save_for_backward(xr, *[P[n] for n in mod.PARAMS], *[t for t in saved if t is not None])
            ctx.mod, ctx.geo = mod, geo
            ctx.shapes, ctx.xshape = [p.shape for p in params], x.shape
        else:
            ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        mod = ctx.mod
        xr, *rest = ctx.saved_tensors
        n = len(mod.PARAMS)
        P, kept = dict(zip(mod.PARAMS, rest[:n])), iter(rest[n:])
        saved = tuple(None if z else next(kept) for z in ctx.none)
        dyr = _as(dy.contiguous().float().view(-1, dy.shape[-1]), xr.dtype)
        dx, grads = mod._bwd(dyr, xr, P, saved, ctx.geo)
        return (None, _as(dx, torch.float32).view(ctx.xshape), None) + _grads(mod.PARAMS, grads, ctx.shapes)


def _apply(mod, x, dim):
    params = [mod.get_parameter(n) for n in mod.PARAMS]
    _check_device(mod, x, params)
    if x.dim() != 3 or x.shape[2] != dim:
        raise ValueError(f"{type(mod).__name__}: x (B, N, {dim}) expected, got {tuple(x.shape)}")
    with torch.cuda.device(x.device):
        return _Function.apply(mod, x, _need(x, params), *params)


def _names(mod):
    return tuple(n for n, _ in mod.named_parameters())


class FeedForward(nn.Module):
    """Position-wise feed forward: dropout(lin2(silu(lin1(x)))).  After a train-mode forward with dropout > 0,
    last_drop_seeds is the int64 device tensor [2] it drew: [0] keys the element mask (seq_ops.residual_dropout's element
    key over the rows [B*N, dim]), [1] is not used."""

    def __init__(self, dim, hidden_dim, dropout=0.1, activation=nn.SiLU, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("FeedForward", compute_dtype)
        if activation is not nn.SiLU:
            raise ValueError("FeedForward: activation nn.SiLU only")
        if dim % 8 or hidden_dim % 8:
            raise ValueError(f"FeedForward: dim and hidden_dim multiples of 8, got {dim} and {hidden_dim}")
        self.lin1 = nn.Linear(dim, hidden_dim)
        self.act = activation()
        self.lin2 = nn.Linear(hidden_dim, dim)
        self.dropout = nn.Dropout(dropout)
        self.compute_dtype = compute_dtype
        self.last_drop_seeds = None
        self.PARAMS = _names(self)

    def _fwd(self, xr, P, xshape):
        y, saved = seq_ops.silu_ffn_fwd(xr, *[P[n] for n in seq_ops.FFN_NAMES])
        drop = None
        if self.training and self.dropout.p > 0:
            self.last_drop_seeds = _draw(2, xr.device)
            drop = (xshape[1], self.last_drop_seeds, float(self.dropout.p), 0.0)
            y = seq_ops.residual_dropout(y, None, *drop)
        return y, saved, drop, xshape

    def _bwd(self, dy, xr, P, saved, drop):
        if drop is not None:
            dy = seq_ops.residual_dropout(dy, None, *drop)
        dx, g = seq_ops.silu_ffn_bwd(dy, xr, P["lin1.weight"], P["lin2.weight"], saved)
        return dx, dict(zip(seq_ops.FFN_NAMES, g))

    def forward(self, x):
        _rates_need_device(self, x, dropout=self.dropout.p)
        return _apply(self, x, self.lin1.in_features)


class ConvModule(nn.Module):
    """LN -> 1x1 conv -> GLU -> depthwise conv -> GroupNorm(1, C) -> SiLU -> 1x1 conv -> dropout -> drop_path -> + x, on
    x [B, N, dim].  After a train-mode forward with a non-zero rate, last_drop_seeds is the int64 device tensor [2] it drew:
    [0] keys the element mask, [1] the drop-path's sample mask (seq_ops.residual_dropout's keys)."""

    def __init__(self, dim, kernel_size=3, dropout=0.1, drop_path=0.0, expansion=1.0, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("ConvModule", compute_dtype)
        if kernel_size % 2 != 1 or not 1 <= kernel_size <= 15:
            raise ValueError(f"ConvModule: kernel_size odd, 1 ... 15, got {kernel_size}")
        hidden_channels = int(dim * expansion)
        if hidden_channels % 2:
            raise ValueError(f"ConvModule: hidden_channels = int(dim * expansion) = {hidden_channels} is odd: the fork's path "
                             "without GLU is not served")
        if dim % 8 or (hidden_channels // 2) % 8:
            raise ValueError(f"ConvModule: dim and the GLU output hidden_channels // 2 multiples of 8, got {dim} and "
                             f"{hidden_channels // 2}")
        self.layer_norm = nn.LayerNorm(dim)
        self.pointwise_conv1 = nn.Conv1d(dim, hidden_channels, kernel_size=1)
        self.glu = nn.GLU(dim=1)
        self.depthwise_conv = nn.Conv1d(hidden_channels // 2, hidden_channels // 2, kernel_size=kernel_size,
                                        padding=kernel_size // 2, groups=hidden_channels // 2, bias=True)
        self.norm = nn.GroupNorm(1, hidden_channels // 2, eps=1e-5)
        self.act = nn.SiLU()
        self.pointwise_conv2 = nn.Conv1d(hidden_channels // 2, dim, kernel_size=1)
        self.dropout = nn.Dropout(dropout)
        self.drop_path = nn.Identity()
        self.drop_path_rate = float(drop_path)
        self.compute_dtype = compute_dtype
        self.last_drop_seeds = None
        self.PARAMS = _names(self)

    def _drop(self, dev):
        if not self.training or not (self.dropout.p > 0 or self.drop_path_rate > 0):
            return None
        self.last_drop_seeds = _draw(2, dev)
        return _site(self.dropout.p, self.drop_path_rate, self.last_drop_seeds)

    def _fwd(self, xr, P, xshape):
        geo = (xshape[0], xshape[1], self._drop(xr.device))
        y, saved = seq_ops.conv_module_fwd(xr, P, geo[0], geo[1], self.layer_norm.eps, self.norm.eps, geo[2])
        return y, saved, geo, xshape

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.conv_module_bwd(dy, xr, P, saved, *geo)

    def forward(self, x):
        _rates_need_device(self, x, dropout=self.dropout.p, drop_path=self.drop_path_rate)
        return _apply(self, x, self.layer_norm.normalized_shape[0])


class Attention(nn.Module):
    """the forks' attention: its parameters and rates; the blocks run it inside their own node"""

    def __init__(self, dim, num_patches, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        if num_heads < 1 or dim % num_heads:
            raise ValueError(f"Attention: dim {dim} is not a multiple of num_heads {num_heads}")
        if dim // num_heads not in HEAD_DIMS:
            raise ValueError(f"Attention: head width {dim // num_heads} (dim / num_heads) outside {HEAD_DIMS}")
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.num_patches = num_patches
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        raise RuntimeError("Attention runs inside ConformerBlock / SqueezeConformerBlock (one autograd node per block)")


class ConformerBlock(nn.Module):
    """x + 1/2 drop_path(FFN) -> x + drop_path(MHSA) -> x + drop_path(ConvModule's branch) -> x + 1/2 drop_path(FFN) ->
    LayerNorm, with dropout ff_dropout behind both feed-forwards and the attention's projection, attn_dropout on the attention
    probabilities and conv_dropout behind the conv branch.

    After a train-mode forward with a non-zero rate, last_drop_seeds is the int64 device tensor [BLOCK_SEEDS = 9] it drew
    (one draw per forward; the backward re-uses it):
        [2 i], [2 i + 1]   site i of SITES = (ffn1, attn, conv, ffn2): the element mask's and the drop-path sample mask's seed,
                           seq_ops.residual_dropout's keys over the rows [B*N, dim]
        [8]                the attention probabilities' mask, the key of seq_ops' `drop=` over [B, heads, N, N]
    A block whose only rate is conv_dropout draws these nine too (before the other rates were served it drew two)."""
    SQUEEZE = False

    def __init__(self, dim, num_heads, num_patches, mlp_ratio=4.0, ff_dropout=0.1, attn_dropout=0.0, conv_dropout=0.0,
                 conv_kernel_size=3, norm_layer=nn.LayerNorm, drop_path=0.0, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype(type(self).__name__, compute_dtype)
        self._build(dim, num_heads, num_patches, mlp_ratio, ff_dropout, attn_dropout, conv_dropout, conv_kernel_size, None,
                    norm_layer, drop_path, compute_dtype)

    def _build(self, dim, num_heads, num_patches, mlp_ratio, ff_dropout, attn_dropout, conv_dropout, conv_kernel_size, se_ratio,
               norm_layer, drop_path, compute_dtype):
        ff_hidden = int(dim * mlp_ratio)
        self.ffn1_norm = norm_layer(dim, elementwise_affine=True)
        self.ffn1 = FeedForward(dim, ff_hidden, dropout=ff_dropout, compute_dtype=compute_dtype)
        self.attn_norm = norm_layer(dim, elementwise_affine=True)
        self.attn = Attention(dim, num_patches, num_heads=num_heads, qkv_bias=True, attn_drop=attn_dropout, proj_drop=ff_dropout)
        self.conv_module = ConvModule(dim, kernel_size=conv_kernel_size, dropout=conv_dropout, compute_dtype=compute_dtype)
        if se_ratio is not None:
            self.se = SqueezeExcite1D(dim, se_ratio, compute_dtype=compute_dtype)
        self.ffn2_norm = norm_layer(dim, elementwise_affine=True)
        self.ffn2 = FeedForward(dim, ff_hidden, dropout=ff_dropout, compute_dtype=compute_dtype)
        self.final_norm = norm_layer(dim, elementwise_affine=True)
        for n in SITES:
            setattr(self, "drop_path_" + n, nn.Identity())
        self.drop_path_rate = float(drop_path)
        self.ff_dropout, self.attn_dropout = float(ff_dropout), float(attn_dropout)
        self.compute_dtype = compute_dtype
        self.last_drop_seeds = None
        self.PARAMS = _names(self)

    def _eps(self):
        return dict(eps=self.ffn1_norm.eps, conv_eps=self.conv_module.layer_norm.eps, gn_eps=self.conv_module.norm.eps)

    def _rates(self):
        """the element-wise rate of each site, in the order of SITES"""
        return (self.ffn1.dropout.p, self.attn.proj_drop.p, self.conv_module.dropout.p, self.ffn2.dropout.p)

    def _regularised(self):
        return self.training and (self.drop_path_rate > 0 or self.attn.attn_drop.p > 0 or any(p > 0 for p in self._rates()))

    def _check_train(self, N):
        """the one combination not served: dropout on the probabilities where the attention pads its token count"""
        p = self.attn.attn_drop.p
        if self.training and p > 0 and seq_ops.plain_attention_pads(self.compute_dtype, N):
            raise NotImplementedError(
                f"{type(self).__name__}: attn_dropout = {p} in train mode at N = {N} tokens is not served: in "
                f"{str(self.compute_dtype).replace('torch.', '')} this N takes the attention route that pads the token count (N off "
                "the 16-byte row), which draws no mask (set attn_dropout to 0, call .eval(), or use a multiple of "
                f"{8 if self.compute_dtype == torch.bfloat16 else 4} tokens)")

    def _check_device_for_rates(self, x):
        ff, _, conv, _ = self._rates()
        _rates_need_device(self, x, ff_dropout=ff, attn_dropout=self.attn.attn_drop.p, conv_dropout=conv,
                           drop_path=self.drop_path_rate)

    def _drops(self, seeds):
        """the BlockDrop of seq_ops over this block's BLOCK_SEEDS seeds; None in eval mode and with every rate zero"""
        if not self._regularised():
            return None
        self.last_drop_seeds = seeds
        sites = [_site(p, self.drop_path_rate, seeds[2 * i:2 * i + 2]) for i, p in enumerate(self._rates())]
        pa = self.attn.attn_drop.p
        return seq_ops.BlockDrop(*sites, probs=(seeds[2 * len(SITES):], float(pa)) if pa > 0 else None)

    def _fwd(self, xr, P, xshape):
        drops = self._drops(_draw(BLOCK_SEEDS, xr.device)) if self._regularised() else None
        geo = (xshape[0], xshape[1], drops)
        y, saved = seq_ops.conformer_block_fwd(xr, P, geo[0], geo[1], self.attn.num_heads, squeeze=self.SQUEEZE,
                                               drops=drops, **self._eps())
        return y, saved, geo, xshape

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.conformer_block_bwd(dy, xr, P, saved, geo[0], geo[1], self.attn.num_heads, squeeze=self.SQUEEZE,
                                           drops=geo[2])

    def forward(self, x):
        if x.dim() == 3:
            self._check_train(x.shape[1])
        self._check_device_for_rates(x)
        return _apply(self, x, self.ffn1_norm.normalized_shape[0])


class SqueezeExcite1D(nn.Module):
    """Squeeze-and-excitation over the tokens of x [B, N, dim]"""

    def __init__(self, dim, se_ratio=0.25, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("SqueezeExcite1D", compute_dtype)
        if dim % 8:
            raise ValueError(f"SqueezeExcite1D: dim a multiple of 8, got {dim}")
        hidden = max(8, int(dim * se_ratio))
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.SiLU()
        self.fc2 = nn.Linear(hidden, dim)
        self.gate = nn.Sigmoid()
        self.compute_dtype = compute_dtype
        self.PARAMS = _names(self)

    def _fwd(self, xr, P, xshape):
        y, saved = seq_ops.se_fwd(xr, P["fc1.weight"], P["fc1.bias"], P["fc2.weight"], P["fc2.bias"], xshape[0], xshape[1])
        return y, saved, xshape[:2], xshape

    def _bwd(self, dy, xr, P, saved, geo):
        dx, g = seq_ops.se_bwd(dy, xr, P["fc1.weight"], P["fc2.weight"], *geo, saved)
        return dx, dict(zip(("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"), g))

    def forward(self, x):
        return _apply(self, x, self.fc1.in_features)


class _Resample(nn.Module):
    PARAMS = ()

    def __init__(self, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype(type(self).__name__, compute_dtype)
        self.compute_dtype = compute_dtype


class Downsample1D(_Resample):
    """length / 2 along the tokens by the mean of each pair (avg_pool1d(2, 2)); N <= 1 is returned as it is"""

    def _fwd(self, xr, P, xshape):
        B, N, D = xshape
        return seq_ops.seq_down2_fwd(xr, B, N), (), (B, N), (B, N // 2, D)

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.seq_down2_bwd(dy, *geo), {}

    def forward(self, x):
        return x if x.shape[1] <= 1 else _apply(self, x, x.shape[2])


class Upsample1D(_Resample):
    """back to target_len tokens by nearest interpolation"""

    def _fwd(self, xr, P, xshape):
        B, n, D = xshape
        zero = torch.zeros(B * self._target, D, dtype=xr.dtype, device=xr.device)
        return seq_ops.seq_up_add_fwd(xr, zero, B, n, self._target), (), (B, n, self._target), (B, self._target, D)

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.seq_up_add_bwd(dy, *geo), {}

    def forward(self, x, target_len):
        if x.shape[1] == target_len:
            return x
        if target_len < x.shape[1]:
            raise ValueError(f"Upsample1D: target_len {target_len} below the {x.shape[1]} tokens of x")
        self._target = int(target_len)
        return _apply(self, x, x.shape[2])


class SqueezeConformerBlock(ConformerBlock):
    """1/2 FFN -> MHSA -> ConvModule -> SE gate -> 1/2 FFN -> LayerNorm"""
    SQUEEZE = True

    def __init__(self, dim, num_heads, num_patches, mlp_ratio=4.0, ff_dropout=0.1, attn_dropout=0.0, conv_dropout=0.1,
                 conv_kernel_size=3, se_ratio=0.25, norm_layer=nn.LayerNorm, drop_path=0.0, compute_dtype=torch.float32):
        nn.Module.__init__(self)
        _check_dtype("SqueezeConformerBlock", compute_dtype)
        self._build(dim, num_heads, num_patches, mlp_ratio, ff_dropout, attn_dropout, conv_dropout, conv_kernel_size, se_ratio,
                    norm_layer, drop_path, compute_dtype)


class SqueezeFormerEncoder(nn.Module):
    """Two-stage SqueezeFormer encoder with one down-sampling and one up-sampling; input and output lengths are equal.
    Block i (stage1, then stage2) takes the drop-path rate linspace(0, drop_path_total, depth)[i], as the fork does.
    After a train-mode forward with a non-zero rate, last_drop_seeds is the int64 device tensor [blocks, BLOCK_SEEDS] of
    one draw: row i is block i's last_drop_seeds (ConformerBlock names the columns)."""

    def __init__(self, dim, num_heads, num_patches, depth, mlp_ratio=4.0, ff_dropout=0.1, attn_dropout=0.0, conv_dropout=0.1,
                 conv_kernel_size=3, se_ratio=0.25, norm_layer=nn.LayerNorm, drop_path_total=0.1, compute_dtype=torch.float32):
        super().__init__()
        _check_dtype("SqueezeFormerEncoder", compute_dtype)
        d1 = max(1, depth // 2)
        d2 = max(1, depth - d1)
        dpr = [x.item() for x in torch.linspace(0, drop_path_total, depth)]
        dpr1, dpr2 = dpr[:d1], dpr[d1:]
        kw = dict(mlp_ratio=mlp_ratio, ff_dropout=ff_dropout, attn_dropout=attn_dropout, conv_dropout=conv_dropout,
                  conv_kernel_size=conv_kernel_size, se_ratio=se_ratio, norm_layer=norm_layer, compute_dtype=compute_dtype)
        self.stage1 = nn.ModuleList([
            SqueezeConformerBlock(dim, num_heads, num_patches, drop_path=dpr1[i] if i < len(dpr1) else 0.0, **kw)
            for i in range(d1)])
        self.down = Downsample1D(compute_dtype)
        self.up = Upsample1D(compute_dtype)
        self.stage2 = nn.ModuleList([
            SqueezeConformerBlock(dim, num_heads, num_patches // 2 if num_patches >= 2 else num_patches,
                                  drop_path=dpr2[i] if i < len(dpr2) else 0.0, **kw)
            for i in range(d2)])
        self.fuse = nn.Identity()
        self.out_norm = norm_layer(dim, elementwise_affine=True)
        self.compute_dtype = compute_dtype
        self.last_drop_seeds = None
        self.PARAMS = _names(self)

    def _blocks(self):
        return list(self.stage1) + list(self.stage2)

    def _fwd(self, xr, P, xshape):
        blocks = self._blocks()
        drops = None
        if any(b._regularised() for b in blocks):
            seeds = _draw(len(blocks) * BLOCK_SEEDS, xr.device).view(len(blocks), BLOCK_SEEDS)
            drops = [b._drops(seeds[i]) for i, b in enumerate(blocks)]
            self.last_drop_seeds = seeds
        geo = (xshape[0], xshape[1], blocks[0].attn.num_heads, len(self.stage1), len(self.stage2), drops)
        y, saved = seq_ops.squeezeformer_fwd(xr, P, *geo[:5], drops=drops, **blocks[0]._eps())
        return y, saved, geo, xshape

    def _bwd(self, dy, xr, P, saved, geo):
        return seq_ops.squeezeformer_bwd(dy, P, saved, *geo[:5], drops=geo[5])

    def forward(self, x):
        if x.dim() == 3:
            N0 = x.shape[1]
            for b in self.stage1:
                b._check_train(N0)
            for b in self.stage2:
                b._check_train(N0 // 2 if N0 > 1 else N0)
        for b in self._blocks():
            b._check_device_for_rates(x)
        return _apply(self, x, self.out_norm.normalized_shape[0])
