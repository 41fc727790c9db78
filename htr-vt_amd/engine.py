"""Host-side execution plan of the HTR-VT hot path on one MI355X.

`Engine.forward` / `Engine.backward` enqueue the gfx950 kernels of
libhtrvt_hip.so in the order of the reference forward
(/root/reference/model_v1/model/HTR_VT.py:222-241, resnet18.py:73-84) and of its
autograd backward (train.py:123).  All arithmetic is in the HIP kernels; torch
only allocates buffers (`torch.empty/zeros`) and provides the stream.

Activation layout: NHWC for the stem, [B,N,D] for tokens, element type
`dtype` (float32 = parity path on f32 MFMA, bfloat16 = throughput path);
statistics, logits, parameters and parameter gradients are float32.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

from . import ops, seq_ops
from ._lib import lib, check, GemmDesc, RelayoutJob, RELAYOUT_PACK_CONV, RELAYOUT_CAST_TRANSPOSE, RELAYOUT_UNPACK_WGRAD, RELAYOUT_ARG_JOBS
from .ops import KMAJOR, MNMAJOR, GATHER_CONV_DGRAD, GATHER_CONV_FWD, GATHER_CONV_WGRAD, ConvGeom, cpad, dt, gemm, ptr, stream

LN_EPS = 1e-6       # HTR_VT.py:252
WHITEN_EPS = 1e-5   # HTR_VT.py:136
BN_EPS = 1e-5       # resnet18.py:16
BN_MOMENTUM = 0.1


def _pool_len(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def stem_tokens(H, W):
    """tokens the ResNet18 stem leaves for an H x W image (resnet18.py:73-84: conv1 s(2,1), max-pool 3 s(2,1) p1,
    layer1 s(2,1), layer2 / layer3 s2, max-pool 3 s(2,1) p1)"""
    h, w = _pool_len(H, 3, 2, 1), W
    h, w = _pool_len(h, 3, 2, 1), _pool_len(w, 3, 1, 1)
    h, w = _pool_len(h, 3, 2, 1), w
    h, w = _pool_len(h, 3, 2, 1), _pool_len(w, 3, 2, 1)
    h, w = _pool_len(h, 3, 2, 1), _pool_len(w, 3, 2, 1)
    h, w = _pool_len(h, 3, 2, 1), _pool_len(w, 3, 1, 1)
    return h * w


# Linear layers of one encoder block per block kind, in the model's named_modules() order (the v1 names whatever attention
# sits between qkv and proj).  A new kind of block is one entry here and one forward / backward pair in Engine._BLOCK.
_V1_LINEARS = ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")
BLOCK_LINEARS = {"full": _V1_LINEARS, "relpos": _V1_LINEARS, "local": _V1_LINEARS,
                 "lgp": ("local_attn.qkv", "local_attn.proj", "global_attn.qkv", "global_attn.proj", "fuse", "mlp.fc1", "mlp.fc2")}

# The stem plan's records.  StemBlock: one residual block (ModelShape.stem_blocks), conv1 has the stride.  BNCoeffs: the
# per-channel float32 vectors of one BatchNorm application, y = x * scale + shift; mean / rstd are what its backward reads.
# SavedBN: one application as its backward needs it: coefficients, parameter prefix, the tensor it normalised.
# ResBlockSaved: what a block's forward keeps: prefix, input x, a1 = relu(bn1(conv1 out)), the output and its 1-bit ReLU
# mask (or None); ConvGeom and SavedBN of conv1 (g1, bn_a), conv2 (g2, bn_b) and the downsample (gd, bn_d; None without one).
# StemGrad: the gradient of a block's output on its way to that block's backward: raw (sums None), or already g = dOut *
# (out > 0) with sums = [(partial, rows)] of the block's bn2 [and downsample BN] from the epilogue of the dgrad that made it.
StemBlock = namedtuple("StemBlock", "prefix Cin planes stride downsample")
BNCoeffs = namedtuple("BNCoeffs", "scale shift mean rstd")
SavedBN = namedtuple("SavedBN", "coef prefix x")
class ResBlockSaved(namedtuple("ResBlockSaved", "p x g1 bn_a a1 g2 bn_b gd bn_d out mask")):
    __slots__ = ()
    __getitem__ = lambda self, name: getattr(self, name)     # by field name, blk["x"]: how the tests and tools read it
StemGrad = namedtuple("StemGrad", "g sums", defaults=(None,))


class ModelShape:
    """Static shape of one model (mirrors MaskedAutoencoderViT.__init__, HTR_VT.py:143-172).  `blocks` states the encoder's
    block list once: per block (kind, arg) = ("full", None), ("relpos", (window, shift)), ("local", (window, shift)) or
    ("lgp", (window, g_tokens, branch_eps)); `relpos` / `local` / `lgp` stay as attributes for the drop-ins and tools."""

    def __init__(self, nb_cls, img_size, embed_dim, depth, num_heads, mlp_ratio=4.0, patch_size=(4, 64), ln_eps=LN_EPS,
                 pos_embed=True, whiten_logits=True, relpos=None, table_patches=None, dropout=False, lgp=None, pos_table=None,
                 local=None, whiten_input=True):
        """The switches of the window-attention fork (model_window/model/HTR_VT.py), defaults = model_v1:
        pos_embed: tokens get the absolute position embedding; whiten_logits: the parameter-free LayerNorm over the logits;
        relpos: None, or per block (window, shift) -- attention with the block's relative-position table
        `blocks.{i}.attn.relative_position_bias_table` [2 table_patches - 1, heads] (window 0: full attention);
        dropout: the model has dropout / drop-path in train mode (not implemented: a train-mode forward is refused).
        The LGP fork (model_lgp/model/plg.py), default None = the blocks above:
        lgp: (window, g_tokens, branch_eps) -- every block is a LocalGlobalParallelBlockSimple: window attention over
        `window` tokens beside attention over min(g_tokens, N) pooled tokens (their LayerNorm without affine at branch_eps),
        fused by a Linear(2D, D); pos_table: float32 [N, D] position embedding the model supplies (the fork keeps it in a
        non-persistent buffer, so no state dict carries it); the token count is what the stem leaves, as for relpos.
        The SGM local-global fork (model_sgm_localglobal/model/HTR_VT.py), default None:
        local: per block None (the v1 full-attention block) or (window, shift) -- a LocalBlock1D: the v1 block with its
        attention inside windows of `window` tokens rolled by `shift` (csrc/lgp.hip; padding slots = the qkv bias, no mask
        across the wrap).  v1 parameter names and the v1 position table `pos_embed`, whose num_patches rows must be the
        tokens the stem leaves (any W that is a multiple of 8 for which the two agree).
        whiten_input: the parameter-free LayerNorm over each input image in front of the stem (HTR_VT.py:224).  False for
        the multi-mask forks model_sgm_mms_attach / _detach, whose forward_features hands the image to the ResNet as it is
        (model_sgm_mms_attach/model/HTR_VT.py:364): the stem kernels then get the statistics (mean 0, rstd 1)."""
        self.nb_cls = int(nb_cls)
        self.whiten_input = bool(whiten_input)
        self.pos_embed, self.whiten_logits, self.dropout = bool(pos_embed), bool(whiten_logits), bool(dropout)
        self.relpos = None if relpos is None else [None if g is None else (int(g[0]), int(g[1])) for g in relpos]
        self.ln_eps = float(ln_eps)
        self.H, self.W = int(img_size[0]), int(img_size[1])
        self.D, self.depth, self.heads = int(embed_dim), int(depth), int(num_heads)
        self.hd = self.D // self.heads
        self.hidden = int(embed_dim * mlp_ratio)
        self.grid = (self.H // patch_size[0], self.W // patch_size[1])
        self.num_patches = self.grid[0] * self.grid[1]
        assert self.D % 32 == 0 and self.D % self.heads == 0
        self.lgp = None if lgp is None else (int(lgp[0]), int(lgp[1]), float(lgp[2]))
        self.local = None if local is None else [None if g is None else (int(g[0]), int(g[1])) for g in local]
        self.pos_table = pos_table
        if self.local is not None:
            if self.relpos is not None or self.lgp is not None:
                raise ValueError("ModelShape: `local` excludes `relpos` and `lgp` (one kind of block list per model)")
            assert len(self.local) == self.depth and self.pos_embed and pos_table is None
            assert all(g is None or 0 <= g[1] < g[0] for g in self.local), "local: 0 <= shift < window"
            assert self.H % 64 == 0 and self.W % 8 == 0, "img_size: H a multiple of 64, W of 8"
            if self.num_patches != stem_tokens(self.H, self.W):
                raise ValueError(f"img_size {self.H} x {self.W} / patch_size {tuple(patch_size)}: the position table has "
                                 f"{self.num_patches} rows, the stem leaves {stem_tokens(self.H, self.W)} tokens")
        elif self.lgp is not None:
            assert self.relpos is None and pos_table is not None
            assert self.H % 64 == 0 and self.W % 8 == 0, "img_size: H a multiple of 64, W of 8"
            self.num_patches = stem_tokens(self.H, self.W)
            assert tuple(pos_table.shape) == (self.num_patches, self.D) and pos_table.dtype == torch.float32
        elif self.relpos is None:
            assert self.H % 64 == 0 and self.W % 64 == 0, "img_size must be a multiple of 64 (HTR_VT.py:158-160)"
        else:   # the window fork has no position grid: the token count is what the stem leaves (any W multiple of 8)
            assert len(self.relpos) == self.depth
            assert self.H % 64 == 0 and self.W % 8 == 0, "img_size: H a multiple of 64, W of 8"
            self.num_patches = stem_tokens(self.H, self.W)
            self.table_patches = int(table_patches if table_patches is not None else self.num_patches)
            assert self.num_patches <= self.table_patches
        if self.lgp is not None:
            self.blocks = [("lgp", self.lgp)] * self.depth
        elif self.local is not None:      # a None entry of either list is the v1 block
            self.blocks = [("full", None) if g is None else ("local", g) for g in self.local]
        elif self.relpos is not None:
            self.blocks = [("full", None) if g is None else ("relpos", g) for g in self.relpos]
        else:
            self.blocks = [("full", None)] * self.depth
        self.kinds = frozenset(kind for kind, _ in self.blocks)

    def stem_blocks(self):
        """the stem's residual blocks in execution order (resnet18.py:52-71): two per stage, the first strided and with a
        1x1 downsample conv + BatchNorm on the residual"""
        D = self.D
        out, inpl = [], D // 4
        for li, (planes, stride) in enumerate(((D // 4, (2, 1)), (D // 2, (2, 2)), (D, (2, 2))), start=1):
            out.append(StemBlock(f"patch_embed.layer{li}.0", inpl, planes, stride, True))
            out.append(StemBlock(f"patch_embed.layer{li}.1", planes, planes, (1, 1), False))
            inpl = planes
        return out

    def stem_convs(self):
        """(param prefix, Ci, Co, k, stride, pad) of every MFMA conv in execution order."""
        out = []
        for b in self.stem_blocks():
            out += [(b.prefix + ".conv1", b.Cin, b.planes, 3, b.stride, 1), (b.prefix + ".conv2", b.planes, b.planes, 3, (1, 1), 1)]
            if b.downsample:
                out.append((b.prefix + ".downsample.0", b.Cin, b.planes, 1, b.stride, 0))
        return out

    def linears(self):
        """parameter prefix of every Linear the engine runs, in the model's named_modules() order"""
        return [f"blocks.{i}.{n}" for i, (kind, _) in enumerate(self.blocks) for n in BLOCK_LINEARS[kind]] + ["head"]


def _job(kind, src, dst0, dst1, d0, d1, taps=0, cpad_in=0, cpad_out=0, row_taps=0, tap0=0):
    j = RelayoutJob()
    j.src, j.dst0, j.dst1, j.kind, j.d0, j.d1 = ptr(src), ptr(dst0), ptr(dst1), kind, d0, d1
    j.taps, j.cpad_in, j.cpad_out, j.row_taps, j.tap0 = taps, cpad_in, cpad_out, row_taps, tap0
    return j


class Engine:
    def __init__(self, shape: ModelShape, dtype=torch.float32, device="cuda", split_bf16=False):
        self.s = shape
        self._stem_blocks, self._stem_convs = shape.stem_blocks(), shape.stem_convs()     # read every step: made once
        self.dtype = dtype
        self.dev = torch.device(device)
        self.dti = dt(dtype)
        # Split-bfloat16 parity path (csrc/split.hip): activations, statistics and every non-GEMM kernel stay float32 exactly
        # as on the float32 path; the convolutions and the encoder's Linear layers -- 98 % of the FLOPs -- run on the bf16
        # matrix cores with operands split into hi + lo bf16 parts concatenated along K (three products, float32
        # accumulate).  `gdt` is the element type the big GEMMs' operands have.
        self.split = bool(split_bf16)
        assert not self.split or dtype == torch.float32, "split_bf16 is a mode of the float32 path"
        for kind, what in (("lgp", "the LGP blocks"), ("local", "local window blocks")):
            if self.split and kind in shape.kinds:
                raise NotImplementedError(f"split_bf16 is not served for {what}: use torch.float32 (parity) or torch.bfloat16")
        self.gdt = torch.bfloat16 if self.split else dtype
        self._split_cache = []       # backward: the few most recent (source tensor, cat, hi, lo) splits (a gradient feeds dgrad AND wgrad)
        self._saved_planes, self._saving = {}, False    # forward(save=True): id(activation) -> its hi / lo planes, for the weight gradients
        self._packs = {}      # name -> (version key, tensors)
        self.weights_epoch = 0   # bumped by whoever rewrites parameters through raw pointers (Trainer.optimizer_step)
        self._unit_stats = None      # whiten_input=False: {mean 0, rstd 1} per image, made once per batch size
        self.fuse_conv1_backward = True   # conv1/bn1/maxpool backward as per-channel sums over the pooled gradient
        self.fuse_bn_backward = True   # bf16: ReLU mask + BN-backward sums in the dgrad epilogue (False: separate pass)
        self.overlap_wgrad = True      # weight-gradient GEMMs on a side stream
        # conv1 + BN + ReLU + max-pool in one pass over the image (no conv1 tensor): the throughput path.  The float32 parity
        # path keeps the two-kernel form by default -- its batch statistics are then summed over the conv outputs the way
        # the reference sums them, which keeps the sign-level comparison of Adam's first updates against the reference
        # trace (tests/test_train_iter_gpu.py) where it was; tests/test_stem_gpu.py runs the fused form in float32 too.
        self.fuse_stem_forward = dtype == torch.bfloat16
        self.fused_attention = True    # bf16: one launch per direction, scores / probabilities never reach HBM (csrc/attention.hip)
        # strided conv dgrad = one launch per input-pixel parity class: independent launches (disjoint output pixels), so
        # they may run on separate streams -- an epilogue-only class (no tap reaches it) then overlaps an MFMA-heavy one
        self.parallel_classes = False
        self._cls_streams = None
        # bf16: every conv / Linear weight is re-packed by ONE table-driven launch per step and the conv weight gradients are
        # unpacked by one launch per DP bucket (csrc/relayout.hip) instead of one launch per tensor (47 per step)
        self.table_relayout = True
        self.relu_mask_from_bn = True   # conv2's fused dgrad epilogue: ReLU mask from the BatchNorm input it reads anyway (no read of a1)
        self.merge_bn_backward = True   # first block of a stage: bn2 + downsample-BN backward in one pass over the shared gradient
        self._pending_unpack = []
        # split-K weight gradients through per-K-range slabs + an ordered sum instead of float atomics: bitwise reproducible
        # run to run (tests/test_determinism_gpu.py).  Round 3: also the bf16 default -- equal to the atomic form at 64-128
        # images per GPU (36.39 vs 36.41 ms), faster below (B = 32: 11.33 vs 11.48 ms, B = 16: 7.22 vs 7.57 ms: float atomics
        # run at ~1.3 TB/s chip-wide, slab stores + the ordered sum at HBM speed)
        self.deterministic = True
        self._side, self._side_active = None, False
        self._call_started = None      # event at the start of the previous forward() (host run-ahead throttle)
        self.capturing = False         # True while Trainer.capture_step records the step into a HIP graph
        # every launch of a step on ONE stream (no weight-gradient / weight-pack side streams): what a captured graph wants
        # on this runtime -- hipGraphLaunch resolves cross-stream edges of a multi-stream capture node by node (measured: a
        # graph of the four-stream step replays SLOWER than the eager launches, 14.3 vs 6.9 ms at 16 images)
        self.single_stream = False
        self.saved = None
        self._bn_train = True
        self._zarena, self._zoff, self._zneed, self._zneed_max = None, None, 0, 0
        self._pos_table, self._zero_pos = None, None     # device copies of the position table the tokens get (_tokens_fwd)

    # ------------------------------------------------------------------ small helpers
    def _empty(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.dtype, device=self.dev)

    def _zeros(self, *shape, dtype=torch.float32):
        """float32 zeros for atomically accumulated outputs.  Inside backward() they are slices of ONE arena cleared by
        one memset per step (31 fill launches otherwise, each with its ~5 us dispatch gap)."""
        if dtype is not torch.float32 or self._zoff is None:
            return torch.zeros(*shape, dtype=dtype, device=self.dev)
        n = 1
        for d in shape:
            n *= int(d)
        n_al = (n + 63) // 64 * 64
        self._zneed += n_al
        if self._zarena is None or self._zoff + n_al > self._zarena.numel():
            return torch.zeros(*shape, dtype=dtype, device=self.dev)
        t = self._zarena[self._zoff:self._zoff + n].view(*shape)
        self._zoff += n_al
        return t

    def _zarena_begin(self):
        if self._zarena is None or self._zarena.numel() < self._zneed_max:
            self._zarena = torch.zeros(max(self._zneed_max, 1), dtype=torch.float32, device=self.dev) if self._zneed_max else None
        elif self._zarena is not None:
            self._zarena.zero_()
        self._zoff, self._zneed = 0, 0

    def _zarena_end(self):
        self._zneed_max = max(self._zneed_max, self._zneed)
        self._zoff = None

    def _wkey(self, t):
        return (t.data_ptr(), t._version, self.weights_epoch)

    # ------------------------------------------------------------------ split-bf16 operands (csrc/split.hip)
    def _split(self, src, rows, cols, order=0, cat=True, planes=False, cat_f32=False, transpose=False):
        """float32 [rows][cols] (contiguous) -> (cat [rows][3 cols] | transposed [cols][3 rows], hi, lo)"""
        BF = torch.bfloat16
        c = None
        if cat:
            shp = (cols, 3 * rows) if transpose else (rows, 3 * cols)
            c = torch.empty(*shp, dtype=torch.float32 if cat_f32 else BF, device=self.dev)
        hi = torch.empty(rows, cols, dtype=BF, device=self.dev) if planes else None
        lo = torch.empty(rows, cols, dtype=BF, device=self.dev) if planes else None
        check(lib.htrvt_split_bf16(ptr(src), rows, cols, cols, ptr(c), order, 1 if cat_f32 else 0, 1 if transpose else 0,
                                   ptr(hi), ptr(lo), stream()), "split_bf16")
        return c, hi, lo

    @staticmethod
    def _batch_slices(B, nbytes, rows_per_image):
        """smallest number of equal batch slices that keeps an operand of `nbytes` below 2 GiB per launch (M tiles of 256
        rows must not straddle slices: the per-tile column sums are concatenated)"""
        def fits(n):
            return B % n == 0 and nbytes // n < 2 ** 31 - 4096 and (n == 1 or (B // n * rows_per_image) % 256 == 0)
        n = 1
        while n < B and not fits(n):
            n += 1
        if not fits(n):
            raise ValueError(f"no batch slicing of {B} images keeps a {nbytes}-byte operand below 2 GiB per launch with whole 256-row tiles "
                             f"({rows_per_image} rows per image)")
        return n

    def _split_act(self, t, cols, cat=True, planes=False):
        """split of an activation / gradient tensor whose innermost extent is `cols`, remembered while the backward may ask
        for it again (the same gradient is the A operand of a dgrad launch and the B operand of three wgrad launches)"""
        cur = torch.cuda.current_stream()
        kept = self._saved_planes.get(id(t))      # a forward that saves for backward split this activation into planes as well
        for ent in self._split_cache + ([kept] if kept is not None else []):
            if ent[0] is t and (ent[1] is not None or not cat) and (ent[2] is not None or not planes):
                if ent[4] != cur:      # made on the main stream, read by a weight-gradient launch on the side stream: the
                    for u in ent[1:4]:  # caching allocator must not hand the block out again before that launch has run
                        if u is not None:
                            u.record_stream(cur)
                return ent[1], ent[2], ent[3]
        want_planes = planes or self._saving      # forward of a training step: the weight gradient will want the planes of this input
        c, hi, lo = self._split(t, t.numel() // cols, cols, order=0, cat=cat, planes=want_planes)
        self._split_cache = [e for e in self._split_cache if e[0] is not t][-2:] + [(t, c, hi, lo, cur)]
        if self._saving:
            self._saved_planes[id(t)] = (t, None, hi, lo, cur)
        return c, hi, lo

    def _lin_w_split(self, name, w):
        """([out][3 in] (hi | hi | lo) for the forward, [in][3 out] of the transposed weight for the dgrad)"""
        key = self._wkey(w)
        ent = self._packs.get(name + "/split")
        if ent is None or ent[0] != key:
            out_f, in_f = w.shape
            ws, _, _ = self._split(w, out_f, in_f, order=1)
            wts, _, _ = self._split(w, out_f, in_f, order=1, transpose=True)
            self._packs[name + "/split"] = (key, (ws, wts))
            return ws, wts
        return ent[1]

    def _conv_w_split(self, name, w):
        """forward pack [Co][taps][Cpad(3 Ci)] and dgrad pack [Ci][taps][Cpad(3 Co)] of the split weight: the conv as seen by
        the bf16 kernels has 3 Ci input channels (hi | hi | lo copies of the weight against (hi | lo | hi) activations)"""
        key = self._wkey(w)
        ent = self._packs.get(name + "/split")
        if ent is None or ent[0] != key:
            Co, Ci, kh, kw = w.shape
            taps = kh * kw
            BF = torch.bfloat16
            cpi3, cpo3 = cpad(3 * Ci, BF), cpad(3 * Co, BF)
            fwd = torch.zeros(Co, taps, cpi3, dtype=BF, device=self.dev)
            dgr = torch.zeros(Ci, taps, cpo3, dtype=BF, device=self.dev)
            v, _, _ = self._split(w, Co, Ci * taps, order=1, cat_f32=True)          # [Co][3][Ci][taps] = a [Co, 3 Ci, kh, kw] weight
            check(lib.htrvt_pack_conv_weight(ptr(v), ptr(fwd), None, Co, 3 * Ci, taps, cpi3, cpad(Co, BF), dt(BF), stream()), "pack_conv_weight")
            v, _, _ = self._split(w, 1, Co * Ci * taps, order=1, cat_f32=True)      # [3][Co][Ci][taps] = a [3 Co, Ci, kh, kw] weight
            check(lib.htrvt_pack_conv_weight(ptr(v), None, ptr(dgr), 3 * Co, Ci, taps, cpad(Ci, BF), cpo3, dt(BF), stream()), "pack_conv_weight")
            self._packs[name + "/split"] = (key, (fwd, dgr))
            return fwd, dgr
        return ent[1]

    def _lin_w(self, name, w):
        """(weight, transposed weight) of a Linear in compute dtype: [out,in] for the forward GEMM and [in,out] for the
        dgrad GEMM dx = dy @ w, so that both are K-major x K-major products on the same kernel.  float32: (w, None)."""
        if self.split:
            return self._lin_w_split(name, w)
        if self.dtype == torch.float32:
            return w, None
        key = self._wkey(w)
        ent = self._packs.get(name)
        if ent is None or ent[0] != key:
            out_f, in_f = w.shape
            bufs = ent[1] if ent is not None else (self._empty(out_f, in_f), self._empty(in_f, out_f))
            check(lib.htrvt_cast_transpose_f32(ptr(w), ptr(bufs[0]), ptr(bufs[1]), out_f, in_f, out_f, self.dti, stream()),
                  "cast_transpose_f32")
            self._packs[name] = (key, bufs)
            return bufs
        return ent[1]

    def _head_w(self, w):
        """head weight in compute dtype, rows zero-padded to a multiple of 8 classes: ([Cp][D], transposed [D][Cp] or None)"""
        C, D = w.shape
        Cp = (C + 7) // 8 * 8
        key = self._wkey(w)
        ent = self._packs.get("head")
        if ent is None or ent[0] != key:
            if self.dtype == torch.float32:
                buf = ent[1][0] if ent is not None else torch.zeros(Cp, D, dtype=self.dtype, device=self.dev)
                buf[:C].copy_(w)          # device memcpy
                bufs = (buf, None)
            else:
                bufs = ent[1] if ent is not None else (torch.zeros(Cp, D, dtype=self.dtype, device=self.dev),
                                                       torch.zeros(D, Cp, dtype=self.dtype, device=self.dev))
                check(lib.htrvt_cast_transpose_f32(ptr(w), ptr(bufs[0]), ptr(bufs[1]), C, D, Cp, self.dti, stream()),
                      "cast_transpose_f32")
            self._packs["head"] = (key, bufs)
            return bufs
        return ent[1]

    def _conv_w(self, name, w):
        """(fwd pack [Co][taps][Cpad_i], dgrad pack [Ci][taps][Cpad_o]) of a conv weight [Co,Ci,k,k]."""
        if self.split:
            return self._conv_w_split(name, w)
        key = self._wkey(w)
        ent = self._packs.get(name)
        Co, Ci, kh, kw = w.shape
        taps = kh * kw
        cpi, cpo = cpad(Ci, self.dtype), cpad(Co, self.dtype)
        if ent is None or ent[0] != key:
            if ent is None:
                fwd = torch.zeros(Co, taps, cpi, dtype=self.dtype, device=self.dev)
                dgr = torch.zeros(Ci, taps, cpo, dtype=self.dtype, device=self.dev)
            else:
                fwd, dgr = ent[1]
            check(lib.htrvt_pack_conv_weight(ptr(w), ptr(fwd), ptr(dgr), Co, Ci, taps, cpi, cpo, self.dti, stream()),
                  "pack_conv_weight")
            self._packs[name] = (key, (fwd, dgr))
            return fwd, dgr
        return ent[1]

    def _conv_w_joint_dgrad(self, name, w3, namd, wd):
        """[Ci][taps + 1][Cpad_o] dgrad pack shared by a block's strided 3x3 conv (tap slots 0 .. taps-1) and its 1x1 downsample
        conv (slot `taps`): the B operand of the parity-class dgrad launches when the downsample gradient rides along as one
        more tap (HtrvtGemmDesc.A2, conv_dgrad(extra=...))."""
        key = (self._wkey(w3), self._wkey(wd))
        ent = self._packs.get(name + "+ds")
        Co, Ci, kh, kw = w3.shape
        taps = kh * kw
        cpi, cpo = cpad(Ci, self.dtype), cpad(Co, self.dtype)
        if ent is None or ent[0] != key:
            buf = ent[1] if ent is not None else torch.zeros(Ci, taps + 1, cpo, dtype=self.dtype, device=self.dev)
            check(lib.htrvt_pack_conv_weight_slots(ptr(w3), None, ptr(buf), Co, Ci, taps, cpi, cpo, taps + 1, 0, self.dti, stream()),
                  "pack_conv_weight_slots")
            check(lib.htrvt_pack_conv_weight_slots(ptr(wd), None, ptr(buf), Co, Ci, 1, cpi, cpo, taps + 1, taps, self.dti, stream()),
                  "pack_conv_weight_slots")
            self._packs[name + "+ds"] = (key, buf)
            return buf
        return ent[1]

    # ------------------------------------------------------------------ GEMM-shaped pieces
    def linear_fwd(self, x, w, bias, out=None, act=0, preact=None, residual=None, c_f32=False):
        M, K = x.shape
        N = w.shape[0]
        if self.split:      # w = (hi | hi | lo) [N][3 K]; float32 in, float32 out
            out = self._empty(M, N) if out is None else out
            xs, _, _ = self._split_act(x, K)
            # the product writes plain float32 + bias (8-phase kernel, 16-byte stores); GELU / saved pre-activation / residual
            # are float32 element-wise passes in the float32 path's order (its GEMM epilogue): v = acc + bias; pre = v;
            # v = gelu(v); v += residual
            first = preact if (act == 1 and preact is not None) else out
            gemm(xs, w, first, dtype=self.gdt, M=M, N=N, K=3 * K, lda=3 * K, ldb=3 * K, ldc=N, bias=bias, c_f32=True)
            if act == 1:
                check(lib.htrvt_elementwise_f32(ptr(first), None, ptr(out), M * N, 0, stream()), "elementwise_f32")
            else:
                assert act == 0 and preact is None
            if residual is not None:
                check(lib.htrvt_elementwise_f32(ptr(out), ptr(residual), ptr(out), M * N, 2, stream()), "elementwise_f32")
            return out
        if out is None:
            out = self._empty(M, N, dtype=torch.float32 if c_f32 else self.dtype)
        gemm(x, w, out, dtype=self.dtype, M=M, N=N, K=K, lda=K, ldb=K, ldc=out.stride(0), bias=bias, act=act, preact=preact,
             residual=residual, c_f32=c_f32)      # (out may be a column block of a wider row-major tensor)
        return out

    def linear_dgrad(self, dy, w, wt=None, act=0, preact=None, plain=False, cols=None):
        """dx[M,K] = dy[M,N] @ w[N,K]  (optionally * gelu'(preact)).  wt = w^T [K][>=N] (bf16 path): K-major B operand.
        cols = (first, N): dy is that column block of a wider row-major tensor (not in split mode)."""
        M, N = dy.shape
        ld, off = N, 0
        if cols is not None:
            assert not self.split
            off, N = cols
        if self.split and not plain:      # wt = (hi | hi | lo) of w^T: [K][3 N]
            K = wt.shape[0]
            dx = self._empty(M, K)
            dys, _, _ = self._split_act(dy, N, cat=True)
            gemm(dys, wt, dx, dtype=self.gdt, M=M, N=K, K=3 * N, lda=3 * N, ldb=3 * N, ldc=K, c_f32=True)
            if act == 2:        # * gelu'(saved pre-activation), float32 element-wise
                check(lib.htrvt_elementwise_f32(ptr(dx), ptr(preact), ptr(dx), M * K, 1, stream()), "elementwise_f32")
            else:
                assert act == 0
            return dx
        K = w.shape[1]
        dx = self._empty(M, K)
        if wt is not None:
            gemm(dy, wt, dx, dtype=self.dtype, M=M, N=K, K=N, lda=ld, ldb=wt.shape[1], ldc=K, act=act, preact=preact, a_off=off)
        else:
            gemm(dy, w, dx, dtype=self.dtype, M=M, N=K, K=N, lda=ld, ldb=K, ldc=K, b_layout=MNMAJOR, act=act, preact=preact,
                 a_off=off)
        return dx

    def _hwgrad_tiles(self, g):
        """(workgroups per pixel range, tile rows, tile columns) of the halo-staged conv weight-gradient kernel
        (csrc/gemm_hwgrad_impl.h: 3x3 stride-1 convolutions), asked of the library itself (htrvt_gemm_wgrad_tiling: the same
        eligibility test htrvt_gemm applies), or None where the generic kernel serves the convolution"""
        if self.gdt != torch.bfloat16:
            return None
        d = GemmDesc()
        cp = cpad(g.Ci, self.gdt)
        d.dtype, d.a_layout, d.b_layout, d.gather = dt(self.gdt), MNMAJOR, MNMAJOR, GATHER_CONV_WGRAD
        d.M, d.N, d.K = g.taps * cp, g.Co, g.B * g.Ho * g.Wo
        d.lda, d.ldb, d.ldc = g.Ci, g.Co, g.Co
        g.fill(d)
        d.Cpad, d.c_f32, d.accumulate, d.batch = cp, 1, 1, 1
        tr, tc = ctypes.c_int32(0), ctypes.c_int32(0)
        n = lib.htrvt_gemm_wgrad_tiling(ctypes.byref(d), ctypes.byref(tr), ctypes.byref(tc))
        return (n, tr.value, tc.value) if n > 0 else None

    def _split_k(self, Mo, No, Kred, conv=False, tiling=None):
        """split-K factor of a weight-gradient GEMM: fill the 256 CUs in whole rounds, but keep the float32
        atomic traffic (one full output tile per block, ~1.3 TB/s chip-wide) small against the MFMA time."""
        bm, bn = (256, 192) if self.gdt == torch.bfloat16 else (128, 128)
        if conv and self.gdt == torch.bfloat16 and No % 256 == 0:
            bn = 256      # gemm_dma.hip pick_bn(): conv weight gradients with N % 256 == 0 use 256x256 tiles
        tiles = ((Mo + bm - 1) // bm) * ((No + bn - 1) // bn)
        if tiling is not None:
            tiles, bm, bn = tiling
        flops = 2.0 * Mo * No * Kred
        best, best_t = 1, None
        # multiples of 8 let the kernel keep all tiles of one K range on one XCD (shared L2); small factors otherwise
        # a single output tile (the 1x1 downsample weight gradients, K = 1 M pixels at layer 1): up to one K range per CU
        smax = 257 if tiles == 1 else 129
        # The conv weight-gradient kernels (gemm_dma_kernel and the gemm_hwgrad kernels) keep the (range, tile) pairs of one XCD
        # consecutive for ANY split factor (xcd_range_map, csrc/gemm_dma_impl.h), so every factor up to 64 is a candidate for
        # them, not only the multiples of 8 and a hand-picked few.  The list is widened for a `tiling` without `conv` too, i.e.
        # the MN-major 8-phase Linear weight-gradient kernel (csrc/gemm8pt_impl.h), which still deals its K ranges over the
        # plain z-grid: there the widened list is unmeasured.
        cands = [1, 2, 3, 4, 5, 6, 7] + list(range(8, smax, 8)) + ([10, 12, 14, 20, 28] if tiling is not None else [])
        if conv or tiling is not None:
            cands = sorted(set(cands) | set(range(8, 65)))
        for s in cands:
            if Kred // s < 512:
                continue
            blocks = tiles * s
            rounds = (blocks + 255) // 256
            # every block's float32 output tile: atomics ~1.3 TB/s chip-wide; slabs are written and read back once at HBM speed
            t = flops / 1.0e15 * (rounds * 256.0 / blocks) + blocks * bm * bn * 4 / (2.5e12 if self.deterministic and s > 1 else 1.3e12)
            if s > 1 and s % 8:
                t *= 1.02     # a K range may straddle two XCDs
            if best_t is None or t < best_t:
                best, best_t = s, t
        return best

    def _splitk_ws(self, sk, Mo, No):
        if sk > 1 and self.deterministic and No % 4:
            if not getattr(self, "_warned_atomics", False):     # slabs need 16-byte rows: this launch falls back to float atomics
                import warnings
                warnings.warn(f"htrvt_amd: split-K weight gradient with {No} output columns (not a multiple of 4) uses float "
                              "atomics: results are not bitwise reproducible although Engine.deterministic is set")
                self._warned_atomics = True
            return None
        if sk <= 1 or not self.deterministic:
            return None
        return self._empty(sk, Mo, No, dtype=torch.float32)

    # Weight gradients have no consumer inside backward: they run on a side stream, overlapping the
    # (HBM-bound) BatchNorm / LayerNorm backward passes and the tails of the dgrad GEMMs on the main stream.
    def _on_side(self, fn, *tensors):
        if not self._side_active:
            return fn()
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        self._side.wait_stream(torch.cuda.current_stream())
        for t in tensors:
            t.record_stream(self._side)      # the caching allocator must not recycle them under the side stream
        with torch.cuda.stream(self._side):
            return fn()

    def _wgrad_stream(self):
        """the stream weight gradients are running on, None when they share the main stream"""
        return self._side if (self._side is not None and self._side_active) else None

    def _join_side(self):
        if self._side is not None and self._side_active:
            torch.cuda.current_stream().wait_stream(self._side)

    def linear_wgrad(self, dy, x, dw, dbias, plain=False, cols=None):
        return self._on_side(lambda: self._linear_wgrad(dy, x, dw, dbias, plain, cols), dy, x)

    def conv_wgrad(self, dy, x, g, dw):
        return self._on_side(lambda: self._conv_wgrad(dy, x, g, dw), dy, x)

    def _linear_wgrad(self, dy, x, dw, dbias, plain=False, cols=None):
        """dw[N,K] += dy^T x ; dbias[N] += colsum(dy).  cols = (first, N): dy is that column block of a wider row-major
        tensor (not in split mode)."""
        M, N = dy.shape
        K = x.shape[1]
        ld, off = N, 0
        if cols is not None:
            assert not self.split
            off, N = cols
        dyp = dy.data_ptr() + off * dy.element_size()
        tiling = None
        if self.gdt == torch.bfloat16 and self.deterministic and not plain:
            # the MN-major 8-phase kernel's 256 x 256 tiles where the LIBRARY says it serves the launch (htrvt_gemm_wgrad_tiling:
            # gemm8pt_serves -- alignment, 2 GiB; no copy of that test here)
            d = GemmDesc()
            d.dtype, d.a_layout, d.b_layout, d.gather = dt(self.gdt), MNMAJOR, MNMAJOR, 0
            d.M, d.N, d.K, d.lda, d.ldb, d.ldc = N, K, M, (3 * N if self.split else ld), K, K
            d.batch, d.split_k, d.c_f32, d.accumulate = 1, 2, 1, 1
            d.A, d.B, d.C = dyp, ptr(x), ptr(dw)
            tr_, tc_ = ctypes.c_int32(0), ctypes.c_int32(0)
            nt = lib.htrvt_gemm_wgrad_tiling(ctypes.byref(d), ctypes.byref(tr_), ctypes.byref(tc_))
            if nt > 0:
                tiling = (nt, tr_.value, tc_.value)
        sk = self._split_k(N, K, M, tiling=tiling)
        if self.split and not plain:      # the contraction runs over the rows: hi / lo planes, three accumulating launches
            # MN-major plain operands carry their own leading dimension: the hi / lo planes of the gradient are column blocks
            # 0 and 1 of the (hi | lo | hi) form the dgrad launch already made -- no second split of dy
            dy3, _, _ = self._split_act(dy, N, cat=True, planes=False)
            _, xh, xl = self._split_act(x, K, cat=False, planes=True)
            for a_off, b_ in ((0, xh), (0, xl), (N, xh)):
                gemm(dy3, b_, dw, dtype=self.gdt, M=N, N=K, K=M, lda=3 * N, ldb=K, ldc=K, a_layout=MNMAJOR, b_layout=MNMAJOR,
                     split_k=sk, accumulate=True, c_f32=True, splitk_ws=self._splitk_ws(sk, N, K), a_off=a_off)
            if dbias is not None:
                ops.colsum(dy, M, N, N, dbias, dti=self.dti)
            return
        gemm(dy, x, dw, dtype=self.dtype, M=N, N=K, K=M, lda=ld, ldb=K, ldc=K, a_layout=MNMAJOR, b_layout=MNMAJOR,
             split_k=sk, accumulate=True, c_f32=True, splitk_ws=self._splitk_ws(sk, N, K), a_off=off)
        if dbias is not None:
            ops.colsum(dyp, M, N, ld, dbias, dti=self.dti)

    def conv_fwd(self, x, wf, g: ConvGeom, want_stats, bn=None, relu=False, residual=None):
        """bn = (scale, shift): eval-mode BatchNorm (running statistics) folded into the launch -- C = relu?(conv * scale +
        shift [+ residual]) -- instead of a raw conv output plus a BatchNorm pass (train mode needs the batch statistics
        of the whole output first)."""
        M = g.B * g.Ho * g.Wo
        cpi = cpad(g.Ci, self.dtype)
        y = self._empty(g.B, g.Ho, g.Wo, g.Co)
        cs, rows = None, 0
        if want_stats:
            rows = ops.gemm_num_mtiles(M, g.Co, self.gdt, gather=GATHER_CONV_FWD)
            cs = self._empty(rows + 64, 2, g.Co, dtype=torch.float32)
        kw = {}
        if bn is not None:
            kw = dict(colscale=bn[0], bias=bn[1], residual=residual, act=3 if relu else 0)
        if self.split:      # the same convolution over 3 Ci input channels: (hi | lo | hi) pixels against the (hi | hi | lo) pack
            x3, _, _ = self._split_act(x, g.Ci)
            cp3 = cpad(3 * g.Ci, self.gdt)
            # the tripled operand of a layer-1 convolution passes 2 GiB at 128 images (the LDS-DMA kernels address operands
            # through 2 GiB buffer descriptors): one launch per batch slice, each with its own rows of the column sums
            n = self._batch_slices(g.B, x3.numel() * 2, g.Ho * g.Wo)
            Bc = g.B // n
            Mc = Bc * g.Ho * g.Wo
            g3 = ConvGeom(Bc, g.Hi, g.Wi, 3 * g.Ci, g.Co, g.kh, (g.sh, g.sw), g.ph)
            rows_c = ops.gemm_num_mtiles(Mc, g.Co, self.gdt, gather=GATHER_CONV_FWD) if want_stats else 0
            if want_stats:
                rows = n * rows_c
                cs = self._empty(rows + 64, 2, g.Co, dtype=torch.float32)
            for c in range(n):
                kc = dict(kw)
                if kc.get("residual") is not None:
                    kc["residual"] = kc["residual"].view(-1)[c * Mc * g.Co:]
                gemm(x3, wf, y, dtype=self.gdt, M=Mc, N=g.Co, K=g.taps * cp3, lda=3 * g.Ci, ldb=g.taps * cp3, ldc=g.Co,
                     gather=GATHER_CONV_FWD, geom=g3, Cpad=cp3, colstats=cs[c * rows_c:] if want_stats else None, c_f32=True,
                     a_off=c * Bc * g.Hi * g.Wi * 3 * g.Ci, c_off=c * Mc * g.Co, **kc)
            return y, cs, rows
        gemm(x, wf, y, dtype=self.dtype, M=M, N=g.Co, K=g.taps * cpi, lda=g.Ci, ldb=g.taps * cpi, ldc=g.Co,
             gather=GATHER_CONV_FWD, geom=g, Cpad=cpi, colstats=cs, **kw)
        return y, cs, rows

    def _dgrad_merged(self, g, dy=None, wd=None, dx=None, extra=None):
        """M tiles of the merged strided-dgrad launch (HtrvtGemmDesc.cls_h = -2) when the library serves `g` in that form
        (asked of the library itself: htrvt_gemm_dgrad_merged_tiles), else 0.  All parity classes of a strided 3x3 conv dgrad
        in ONE launch on halo-staged tiles (csrc/gemm_halo_impl.h, gemm_halo_s2_kernel) instead of one gather launch per class"""
        if not (self.gdt == torch.bfloat16 and not self.split and self._dgrad_by_class(g) and g.kh == 3):
            return 0
        d = GemmDesc()
        cpo = cpad(g.Co, self.dtype)
        d.dtype, d.a_layout, d.b_layout, d.gather = dt(self.dtype), KMAJOR, KMAJOR, GATHER_CONV_DGRAD
        d.M, d.N, d.K = g.B * g.Hi * g.Wi, g.Ci, (g.taps + (1 if extra is not None else 0)) * cpo
        d.lda, d.ldb, d.ldc = g.Co, (g.taps + (1 if extra is not None else 0)) * cpo, g.Ci
        g.fill(d)
        d.Cpad, d.batch, d.split_k, d.cls_h, d.cls_w = cpo, 1, 1, -2, -2
        # the pointer tests of the eligibility check (alignment, A2 behind A): the real ones when known, aligned stand-ins else
        d.A = ptr(dy) if dy is not None else 4096
        d.B = ptr(wd) if wd is not None else 4096
        d.C = ptr(dx) if dx is not None else 4096
        d.A2 = ptr(extra)
        return int(lib.htrvt_gemm_dgrad_merged_tiles(ctypes.byref(d)))

    def dgrad_tiles(self, g: ConvGeom):
        """number of M tiles (rows of a fused BN-backward partial buffer) conv_dgrad will produce"""
        nm = self._dgrad_merged(g)
        if nm > 0:
            return nm
        if self._dgrad_by_class(g):
            return sum(ops.gemm_num_mtiles(g.B * Hq * Wq, g.Ci, self.dtype, gather=GATHER_CONV_DGRAD)
                       for _a, _b, _nt, Hq, Wq in g.parity_classes())
        return ops.gemm_num_mtiles(g.B * g.Hi * g.Wi, g.Ci, self.dtype, gather=GATHER_CONV_DGRAD)

    def _dgrad_by_class(self, g):
        return self.gdt == torch.bfloat16 and (g.sh, g.sw) != (1, 1) and g.B * g.Hi * g.Wi // (g.sh * g.sw) > 128

    def conv_dgrad(self, dy, wd, g: ConvGeom, residual=None, relu_src=None, bnb=None, extra=None, relu_bn=None, relu_bits=False):
        """dx = conv-dgrad(dy) [+ residual] [masked by relu_src > 0]; bnb: fused BatchNorm-backward sums (bf16 only).
        extra = dy2 (parity-class path only): the gradient of the block's 1x1 downsample conv output, allocated right
        behind dy; wd is then the joint pack of _conv_w_joint_dgrad and dx also receives the 1x1 conv's input gradient."""
        cpo = cpad(g.Co, self.dtype)
        dx = self._empty(g.B, g.Hi, g.Wi, g.Ci)
        assert extra is None or self._dgrad_by_class(g)
        assert relu_bn is None or (not self._dgrad_by_class(g) and relu_src is None and residual is None and bnb is not None and len(bnb) == 1)
        wtaps = g.taps + (1 if extra is not None else 0)       # taps per row of the packed weight
        if self._dgrad_by_class(g) and self.split:
            # split-bf16: the same parity-class launches over 3 Co gradient channels; each leaves a dense float32 [B,Hq,Wq,Ci]
            # matrix (the float32 epilogue of the LDS-DMA kernels stores class rows as they come), one pass interleaves the
            # classes into dx and adds the residual (htrvt_class_scatter_f32)
            assert relu_src is None and bnb is None and relu_bn is None and extra is None
            dy3, _, _ = self._split_act(dy, g.Co, cat=True, planes=True)
            cp3 = cpad(3 * g.Co, self.gdt)
            g3 = ConvGeom(g.B, g.Hi, g.Wi, g.Ci, 3 * g.Co, g.kh, (g.sh, g.sw), g.ph)
            parts = {}
            for a, b, nt, Hq, Wq in g.parity_classes():
                if nt == 0:      # no tap reaches this class (1x1 strided conv): its gradient is zero
                    parts[(a, b)] = torch.zeros(g.B, Hq, Wq, g.Ci, dtype=torch.float32, device=self.dev)
                    continue
                part = self._empty(g.B, Hq, Wq, g.Ci)
                # cls selects the taps and the gathered pixels; with cls the float32 epilogue writes row m of the class
                # at row m of C: a dense matrix
                gemm(dy3, wd, part, dtype=self.gdt, M=g.B * Hq * Wq, N=g.Ci, K=nt * cp3, lda=3 * g.Co, ldb=g.taps * cp3, ldc=g.Ci,
                     gather=GATHER_CONV_DGRAD, geom=g3, Cpad=cp3, cls=(a, b), c_f32=True)
                parts[(a, b)] = part
            check(lib.htrvt_class_scatter_f32(ptr(parts[(0, 0)]), ptr(parts.get((0, 1))), ptr(parts.get((1, 0))), ptr(parts.get((1, 1))),
                                              ptr(residual), ptr(dx), g.B, g.Hi, g.Wi, g.Ci, g.sh, g.sw, stream()), "class_scatter_f32")
            return dx
        if self._dgrad_merged(g, dy, wd, dx, extra) > 0:
            # strided 3x3 conv: every parity class in one launch, halo-staged tiles; the downsample gradient rides along (A2)
            gemm(dy, wd, dx, dtype=self.dtype, M=g.B * g.Hi * g.Wi, N=g.Ci, K=wtaps * cpo, lda=g.Co, ldb=wtaps * cpo, ldc=g.Ci,
                 gather=GATHER_CONV_DGRAD, geom=g, Cpad=cpo, residual=residual, cls=(-2, -2), relu_src=relu_src,
                 relu_bits=relu_bits, bnb=bnb, a2=extra)
            return dx
        if self._dgrad_by_class(g):
            # strided conv: one launch per input-pixel parity class, each contracting only the taps that reach it
            tile0 = 0
            par = self.parallel_classes and ops.PROFILE is None
            main = torch.cuda.current_stream()
            if par and self._cls_streams is None:
                self._cls_streams = [torch.cuda.Stream(device=self.dev) for _ in range(3)]
            used = []
            for a, b, nt, Hq, Wq in g.parity_classes():
                idx = a * g.sw + b
                st_ = self._cls_streams[idx - 1] if (par and idx > 0) else main
                if st_ is not main:
                    st_.wait_stream(main)
                    used.append(st_)
                a2 = extra if (extra is not None and (a, b) == (0, 0)) else None    # the pixels a 1x1 stride-s conv reads
                with torch.cuda.stream(st_):
                    gemm(dy, wd, dx, dtype=self.dtype, M=g.B * Hq * Wq, N=g.Ci, K=(nt + (1 if a2 is not None else 0)) * cpo,
                         lda=g.Co, ldb=wtaps * cpo, ldc=g.Ci, gather=GATHER_CONV_DGRAD, geom=g, Cpad=cpo, residual=residual,
                         cls=(a, b), relu_src=relu_src, relu_bits=relu_bits, bnb=bnb, bnb_tile0=tile0, a2=a2)
                tile0 += ops.gemm_num_mtiles(g.B * Hq * Wq, g.Ci, self.dtype, gather=GATHER_CONV_DGRAD)
            for st_ in used:       # every class has written its pixels before anything downstream reads dx
                main.wait_stream(st_)
            return dx
        if self.split:      # 3 Co gradient channels: (hi | lo | hi) against the (hi | hi | lo) dgrad pack
            assert relu_src is None and bnb is None and relu_bn is None
            dy3, _, _ = self._split_act(dy, g.Co, cat=True, planes=True)
            cp3 = cpad(3 * g.Co, self.gdt)
            n = self._batch_slices(g.B, dy3.numel() * 2, g.Hi * g.Wi)
            Bc = g.B // n
            Mc = Bc * g.Hi * g.Wi
            g3 = ConvGeom(Bc, g.Hi, g.Wi, g.Ci, 3 * g.Co, g.kh, (g.sh, g.sw), g.ph)
            for c in range(n):
                gemm(dy3, wd, dx, dtype=self.gdt, M=Mc, N=g.Ci, K=g.taps * cp3, lda=3 * g.Co, ldb=g.taps * cp3,
                     ldc=g.Ci, gather=GATHER_CONV_DGRAD, geom=g3, Cpad=cp3,
                     residual=None if residual is None else residual.view(-1)[c * Mc * g.Ci:], c_f32=True,
                     a_off=c * Bc * g.Ho * g.Wo * 3 * g.Co, c_off=c * Mc * g.Ci)
            return dx
        gemm(dy, wd, dx, dtype=self.dtype, M=g.B * g.Hi * g.Wi, N=g.Ci, K=g.taps * cpo, lda=g.Co, ldb=g.taps * cpo,
             ldc=g.Ci, gather=GATHER_CONV_DGRAD, geom=g, Cpad=cpo, residual=residual, relu_src=relu_src, relu_bits=relu_bits, bnb=bnb,
             relu_bn=relu_bn)
        return dx

    def _conv_wgrad(self, dy, x, g: ConvGeom, dw):
        M = g.B * g.Ho * g.Wo
        cpi = cpad(g.Ci, self.gdt)
        packed = self._zeros(g.taps, cpi, g.Co)
        sk = self._split_k(g.taps * cpi, g.Co, M, conv=True, tiling=self._hwgrad_tiles(g))
        if self.split:      # the contraction runs over the pixels: hi / lo planes, three accumulating launches
            _, xh, xl = self._split_act(x, g.Ci, cat=False, planes=True)
            _, dyh, dyl = self._split_act(dy, g.Co, cat=False, planes=True)
            pairs = ((xh, dyh), (xl, dyh), (xh, dyl))
        else:
            pairs = ((x, dy),)
        for x_, dy_ in pairs:
            gemm(x_, dy_, packed, dtype=self.gdt, M=g.taps * cpi, N=g.Co, K=M, lda=g.Ci, ldb=g.Co, ldc=g.Co,
                 a_layout=MNMAJOR, b_layout=MNMAJOR, gather=GATHER_CONV_WGRAD, geom=g, Cpad=cpi,
                 split_k=sk, accumulate=True, c_f32=True, splitk_ws=self._splitk_ws(sk, g.taps * cpi, g.Co))
        if self.table_relayout and self._zoff is not None:    # inside backward(): unpacked with its DP bucket, one launch
            self._pending_unpack.append((packed, dw, g.Co, g.Ci, g.taps, cpi))
        else:
            check(lib.htrvt_unpack_conv_wgrad(ptr(packed), ptr(dw), g.Co, g.Ci, g.taps, cpi, stream()), "unpack_conv_wgrad")

    def _flush_unpacks(self):
        """grad [Co][Ci][taps] += every pending conv weight-gradient GEMM output, one launch, on the stream that produced them"""
        if not self._pending_unpack:
            return
        pend, self._pending_unpack = self._pending_unpack, []

        def run():
            self._relayout([_job(RELAYOUT_UNPACK_WGRAD, packed, dw, None, Co, Ci, taps, cpi) for packed, dw, Co, Ci, taps, cpi in pend])
        self._on_side(run)

    # ------------------------------------------------------------------ table-driven re-layouts (csrc/relayout.hip)
    def _relayout(self, jobs):
        """run RelayoutJobs, <= 48 per launch: the table is planned on the host and travels in the kernel-argument segment
        (no device copy to keep alive, nothing to refresh when autograd hands out new gradient buffers)"""
        for i in range(0, len(jobs), RELAYOUT_ARG_JOBS):
            chunk = jobs[i:i + RELAYOUT_ARG_JOBS]
            arr = (RelayoutJob * len(chunk))(*chunk)
            total = lib.htrvt_relayout_plan(arr, len(chunk))
            if total < 0:
                raise RuntimeError(lib.htrvt_last_error().decode())
            check(lib.htrvt_relayout_host(arr, len(chunk), total, self.dti, stream()), "relayout")

    def _repack_all(self, P, save):
        """bf16: refresh every stale conv pack / Linear copy in one launch (what _conv_w / _conv_w_joint_dgrad / _lin_w /
        _head_w would do one tensor at a time on their first use after an optimizer step)."""
        s = self.s
        jobs, fresh = [], []
        for name, _ci, _co, _k, _st, _pd in self._stem_convs:
            w = P[name + ".weight"]
            key, ent = self._wkey(w), self._packs.get(name)
            if ent is not None and ent[0] == key:
                continue
            Co, Ci, kh, kw = w.shape
            taps, cpi, cpo = kh * kw, cpad(Ci, self.dtype), cpad(Co, self.dtype)
            bufs = ent[1] if ent is not None else (torch.zeros(Co, taps, cpi, dtype=self.dtype, device=self.dev),
                                                   torch.zeros(Ci, taps, cpo, dtype=self.dtype, device=self.dev))
            jobs.append(_job(RELAYOUT_PACK_CONV, w, bufs[0], bufs[1], Co, Ci, taps, cpi, cpo, taps, 0))
            fresh.append((name, key, bufs))
        for pb in (b.prefix for b in self._stem_blocks if save and b.downsample):     # the joint dgrad packs
            w3, wd = P[pb + ".conv1.weight"], P[pb + ".downsample.0.weight"]
            key, ent = (self._wkey(w3), self._wkey(wd)), self._packs.get(pb + ".conv1+ds")
            if ent is not None and ent[0] == key:
                continue
            Co, Ci, kh, kw = w3.shape
            taps, cpi, cpo = kh * kw, cpad(Ci, self.dtype), cpad(Co, self.dtype)
            buf = ent[1] if ent is not None else torch.zeros(Ci, taps + 1, cpo, dtype=self.dtype, device=self.dev)
            jobs.append(_job(RELAYOUT_PACK_CONV, w3, None, buf, Co, Ci, taps, cpi, cpo, taps + 1, 0))
            jobs.append(_job(RELAYOUT_PACK_CONV, wd, None, buf, Co, Ci, 1, cpi, cpo, taps + 1, taps))
            fresh.append((pb + ".conv1+ds", key, buf))
        for name in s.linears():
            w = P[name + ".weight"]
            key, ent = self._wkey(w), self._packs.get(name)
            if ent is not None and ent[0] == key:
                continue
            out_f, in_f = w.shape
            ld_t = (out_f + 7) // 8 * 8 if name == "head" else out_f     # head: classes zero-padded to a multiple of 8
            if ent is not None:
                bufs = ent[1]
            elif name == "head":
                bufs = (torch.zeros(ld_t, in_f, dtype=self.dtype, device=self.dev), torch.zeros(in_f, ld_t, dtype=self.dtype, device=self.dev))
            else:
                bufs = (self._empty(out_f, in_f), self._empty(in_f, out_f))
            jobs.append(_job(RELAYOUT_CAST_TRANSPOSE, w, bufs[0], bufs[1], out_f, in_f, 0, ld_t))
            fresh.append((name, key, bufs))
        if jobs:
            self._relayout(jobs)
            for name, key, bufs in fresh:
                self._packs[name] = (key, bufs)

    # ------------------------------------------------------------------ BatchNorm pieces
    def bn_coeffs(self, P, prefix, C, train, cs=None, rows=0, count=0, save=False):
        """returns BNCoeffs (scale, shift, save_mean, save_rstd)"""
        scale, shift = self._empty(C, dtype=torch.float32), self._empty(C, dtype=torch.float32)
        if train:
            mean, rstd = self._empty(C, dtype=torch.float32), self._empty(C, dtype=torch.float32)
            check(lib.htrvt_bn_finalize(ptr(cs), rows, C, float(count), ptr(P[prefix + ".weight"]), ptr(P[prefix + ".bias"]),
                                        BN_EPS, BN_MOMENTUM, ptr(P[prefix + ".running_mean"]),
                                        ptr(P[prefix + ".running_var"]), ptr(P[prefix + ".num_batches_tracked"]),
                                        ptr(scale), ptr(shift), ptr(mean), ptr(rstd), stream()), "bn_finalize")
            return BNCoeffs(scale, shift, mean, rstd)
        # eval mode (running statistics).  save: an eval-mode backward (frozen-BN fine-tuning, saliency) needs them as
        # (mean, rstd); they are constants there, bn_backward_finish is told so through self._bn_train
        rstd = self._empty(C, dtype=torch.float32) if save else None
        check(lib.htrvt_bn_eval_coeffs(ptr(P[prefix + ".weight"]), ptr(P[prefix + ".bias"]), ptr(P[prefix + ".running_mean"]),
                                       ptr(P[prefix + ".running_var"]), BN_EPS, ptr(scale), ptr(shift), ptr(rstd), C, stream()),
              "bn_eval_coeffs")
        return BNCoeffs(scale, shift, P[prefix + ".running_mean"] if save else None, rstd)

    def bn_apply(self, x, scale, shift, relu, res=None, rscale=None, rshift=None, want_mask=False):
        """y = [relu](x * scale + shift [+ res [* rscale + rshift]]); want_mask: also the 1-bit-per-element sign mask of y
        (uint8 [numel / 8]) that the backward of this ReLU reads instead of y (HtrvtGemmDesc.relu_bits)"""
        y = torch.empty_like(x)
        C = x.shape[-1]
        if want_mask:
            mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device)
            check(lib.htrvt_bn_apply_mask(ptr(x), ptr(scale), ptr(shift), ptr(res), ptr(rscale), ptr(rshift), ptr(y), ptr(mask),
                                          x.numel() // C, C, 1 if relu else 0, self.dti, stream()), "bn_apply_mask")
            return y, mask
        check(lib.htrvt_bn_apply(ptr(x), ptr(scale), ptr(shift), ptr(res), ptr(rscale), ptr(rshift), ptr(y),
                                 x.numel() // C, C, 1 if relu else 0, self.dti, stream()), "bn_apply")
        return y

    def bn_backward(self, dy, yact, bn, P, G, want_g=False, out=None):
        """dx of the train-mode BatchNorm `bn` (SavedBN) (+ReLU mask from yact); accumulates dgamma/dbeta into G.  Unfused
        form: one reduction pass over (dy, yact, x), then bn_backward_finish."""
        C = bn.x.shape[-1]
        npix = bn.x.numel() // C
        nblk = lib.htrvt_bn_bwd_blocks(npix)
        partial = self._empty(nblk, 2, C, dtype=torch.float32)
        check(lib.htrvt_bn_bwd_reduce(ptr(dy), ptr(yact), ptr(bn.x), ptr(bn.coef.mean), ptr(bn.coef.rstd), ptr(partial), npix, C,
                                      self.dti, stream()), "bn_bwd_reduce")
        return self.bn_backward_finish(partial, nblk, dy, yact, bn, P, G, want_g, out=out)

    def bn_backward_coef(self, partial, rows, bn, P, G):
        """finalize dgamma / dbeta (accumulated into G) and the [3][C] coefficients of dx = cA*g + cB*x + cC from per-tile
        partial sums"""
        C = bn.x.shape[-1]
        coef = self._empty(3, C, dtype=torch.float32)
        if rows > 64:   # two-level reduction of the partial rows
            red = self._zeros(2 * C)
            ops.colsum(partial, rows, 2 * C, 2 * C, red, dti=0)
            partial, rows = red, 1
        count = float(bn.x.numel() // C) if self._bn_train else -1.0      # eval mode: dx = gamma * rstd * g
        check(lib.htrvt_bn_bwd_finalize(ptr(partial), rows, C, count, ptr(P[bn.prefix + ".weight"]), ptr(bn.coef.mean),
                                        ptr(bn.coef.rstd), ptr(G[bn.prefix + ".weight"]), ptr(G[bn.prefix + ".bias"]), ptr(coef),
                                        stream()), "bn_bwd_finalize")
        return coef

    def bn_backward_finish(self, partial, rows, g, yact, bn, P, G, want_g=False, out=None):
        """finalize (dgamma, dbeta, coefficients) from per-tile partial sums, then dx = cA*g + cB*x + cC.
        With yact=None, g is the already ReLU-masked gradient (fused dgrad epilogue)."""
        x = bn.x
        C = x.shape[-1]
        coef = self.bn_backward_coef(partial, rows, bn, P, G)
        dx = torch.empty_like(x) if out is None else out
        gout = torch.empty_like(x) if want_g else None
        check(lib.htrvt_bn_bwd_apply(ptr(g), ptr(yact), ptr(x), ptr(coef), ptr(dx), ptr(gout), x.numel() // C, C, self.dti,
                                     stream()), "bn_bwd_apply")
        return dx, gout

    def _bnb_request(self, bns, rows):
        """fused BatchNorm-backward sums of a conv_dgrad with `rows` M tiles, for the BatchNorms `bns` its output gradient
        feeds: (conv_dgrad's bnb list [(x, mean, rstd, partial)], [(partial [rows, 2, C], rows)])"""
        bufs = [self._empty(rows, 2, bn.x.shape[-1], dtype=torch.float32) for bn in bns]
        return [(bn.x, bn.coef.mean, bn.coef.rstd, b) for bn, b in zip(bns, bufs)], [(b, rows) for b in bufs]

    # ------------------------------------------------------------------ LayerNorm pieces
    def ln_fwd(self, P, name, x, save):
        return seq_ops.layernorm_fwd(x, P[name + ".weight"], P[name + ".bias"], self.s.ln_eps, save)

    def ln_bwd(self, P, G, name, dy, x, mean, rstd, dres):
        return seq_ops.layernorm_bwd(dy, x, mean, rstd, P[name + ".weight"], G[name + ".weight"], G[name + ".bias"], dres)

    # ------------------------------------------------------------------ forward
    def forward(self, P, img, keep_mask=None, train=False, save=False, want_features=False):
        """P: dict name -> float32 device tensor (parameters and BN buffers, reference state_dict names).
        img: [B,1,H,W] float32.  keep_mask: None, [N] (1 keep / 0 mask-token, one mask for the batch) or [B,N] / [B,N,1]
        (one mask per image, the multi-mask forks); any other shape is a ValueError.
        Returns float32 logits [B,N,nb_cls] (after the final param-free LayerNorm); want_features: (logits, feats) with
        feats the final norm's output as a fresh float32 [B,N,D] tensor (the SGM forks' feature tap)."""
        B, u8, keep = self._begin_forward(img, keep_mask, train, want_features)
        sv = {} if save else None
        self._split_cache = []
        self._saved_planes, self._saving = {}, bool(save) and self.split
        prefetched = self._prefetch_weights(P, save)
        x, Hc, Wc = self._stem_fwd(P, img, u8, train, save, sv, prefetched)
        tok, N = self._tokens_fwd(P, x, keep, B, Hc, Wc, sv)
        xt, enc_saved = self._encoder_fwd(P, tok.view(B * N, self.s.D), B, N, save)
        y, feats = self._head_fwd(P, xt, B, N, train, sv, want_features)
        self._saving = False
        if save:
            sv["enc"] = enc_saved
            self.saved = sv
        return (y, feats) if want_features else y

    def _begin_forward(self, img, keep_mask, train, want_features):
        """argument checks, the host run-ahead throttle and the upload of the span mask: (B, uint8 pixels?, keep on the device)"""
        s = self.s
        if want_features and self.split:
            raise NotImplementedError("split_bf16 has no feature output: use compute_dtype=torch.float32 (parity) or "
                                      "torch.bfloat16")
        if want_features and "lgp" in s.kinds:
            raise NotImplementedError("want_features is not served for the LGP model")
        if train and s.dropout:
            raise NotImplementedError("train-mode forward of a model with dropout / drop-path: not implemented (build the "
                                      "window model with create_model(..., dropout=False) to train without them)")
        assert img.is_cuda and img.dtype in (torch.float32, torch.uint8) and img.is_contiguous()
        u8 = 1 if img.dtype == torch.uint8 else 0    # uint8 pixels are read as value / 255 (ToTensor) by the first kernels
        B, _, H, W = img.shape
        assert (H, W) == (s.H, s.W), f"model built for {s.H}x{s.W}, got {H}x{W}"
        # Host run-ahead throttle: enqueueing a step takes ~6 ms of host time against ~40 ms on the device, and nothing in
        # a step makes the host wait.  Unbounded, the host queues many steps; every step's activations are then alive at
        # once (the caching allocator cannot reuse a block before the streams that touched it have passed its
        # record_stream events), the pool grows from 20 to ~96 GiB and the hundreds of device allocations that takes land
        # in the middle of the run (measured: 120 ms per step for the first ten steps after warm-up).  So: before
        # enqueueing call k the host waits until the device has STARTED call k-1 -- one call of run-ahead, which is all
        # the device needs to never run dry.
        # (while a HIP graph is being captured -- Trainer.capture_step -- nothing may wait on the host and there is no
        # run-ahead to bound: the replaying caller throttles itself)
        if not self.capturing:
            if self._call_started is not None:
                self._call_started.synchronize()
            self._call_started = torch.cuda.Event()
            self._call_started.record()
        keep = None
        if keep_mask is not None:   # uploaded before anything is enqueued: a pageable host->device copy waits for the stream
            N = s.num_patches
            shape = tuple(keep_mask.shape)
            if shape not in ((N,), (B, N), (B, N, 1)):
                raise ValueError(f"keep_mask of shape {shape}: expected [{N}] (one mask for the batch), or [{B}, {N}] / "
                                 f"[{B}, {N}, 1] (one mask per image of this batch of {B})")
            keep = keep_mask.to(dtype=torch.float32).contiguous()
            if len(shape) > 1:      # per-sample rows (the multi-mask forks): _tokens_fwd / _tokens_bwd see keep.dim() == 2
                keep = keep.view(B, N)
            if not keep.is_cuda:    # through pinned memory: a pageable copy would make the host wait for the previous step
                keep = keep.pin_memory().to(self.dev, non_blocking=True)
        return B, u8, keep

    def _prefetch_weights(self, P, save):
        """training steps rewrite every weight: re-pack / re-cast all of them on the side stream at the start of the forward,
        under the (HBM-bound) image statistics, conv1 and max-pool kernels, instead of ~30 latency-bound launches in
        front of their first use.  True when the side stream has work the stem must wait for."""
        if self.dtype == torch.bfloat16 and self.single_stream:
            if self.table_relayout:
                self._repack_all(P, save)
        elif self.dtype == torch.bfloat16:
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.dev)
            self._side.wait_stream(torch.cuda.current_stream())     # behind whatever wrote the weights (the optimizer step)
            with torch.cuda.stream(self._side):
                if self.table_relayout:
                    self._repack_all(P, save)
                else:
                    for name, _ci, _co, _k, _st, _pd in self._stem_convs:
                        self._conv_w(name, P[name + ".weight"])
                    for pb in (b.prefix for b in self._stem_blocks if save and b.downsample):
                        self._conv_w_joint_dgrad(pb + ".conv1", P[pb + ".conv1.weight"], pb + ".downsample.0", P[pb + ".downsample.0.weight"])
                    for name in self.s.linears():
                        if name == "head":
                            self._head_w(P["head.weight"])
                        else:
                            self._lin_w(name, P[name + ".weight"])
            return True
        return False

    def _stem_fwd(self, P, img, u8, train, save, sv, prefetched):
        """the ResNet18 stem up to the layer-3 output: (x [B,Hc,Wc,D], Hc, Wc)"""
        x = self._stem_head_fwd(P, img, u8, train, save, sv)
        if prefetched:
            torch.cuda.current_stream().wait_stream(self._side)
        # --- residual stages (resnet18.py:79-81, 23-39) ---
        block_fwd = self._res_block_fwd if (train or save) else self._res_block_fwd_eval
        blocks_saved = []
        for b in self._stem_blocks:
            x, blk = block_fwd(P, b, x, train, save)
            blocks_saved.append(blk)
        if save:
            sv["stem_blocks"] = blocks_saved
        return x, x.shape[1], x.shape[2]

    def _stem_head_fwd(self, P, img, u8, train, save, sv):
        """whitening statistics + conv1 + BN + ReLU + maxpool (resnet18.py:74-77): the pooled activations [B,Hp,W,D/4]"""
        st, C1 = stream(), self.s.D // 4
        B, _, H, W = img.shape
        if self.s.whiten_input:
            stats = self._empty(B, 2, dtype=torch.float32)
            check(lib.htrvt_img_stats(ptr(img), ptr(stats), B, H * W, WHITEN_EPS, u8, st), "img_stats")
        else:       # the kernels whiten with (pixel - mean) * rstd: {0, 1} per image leaves the pixels as they are
            if self._unit_stats is None or self._unit_stats.shape[0] != B:
                self._unit_stats = torch.tensor([0.0, 1.0], device=self.dev).repeat(B, 1)
            stats = self._unit_stats
        w1 = P["patch_embed.conv1.weight"]
        Hp = (H // 2 - 1) // 2 + 1
        a = self._empty(B, Hp, W, C1)
        idx = torch.empty(B, Hp, W, C1, dtype=torch.uint8, device=self.dev) if save else None
        # The conv1 tensor (1.6 GB at the bench shape) is needed only by the unfused backward of the stem; otherwise
        # conv1 + BatchNorm + ReLU + max-pool run as ONE pass over the image, the batch statistics of a train-mode
        # BatchNorm coming from the image's second moments (csrc/stem.hip: stem_moments / stem_stats / stem_fused_fwd).
        fused_stem = self.fuse_stem_forward and (not save or (train and self.fuse_conv1_backward))
        if fused_stem:
            c1, cs = None, None
            if train:
                cs = self._empty(2, C1, dtype=torch.float32)
                part = self._empty(lib.htrvt_stem_stats_rows(B, H), 64, dtype=torch.float32)
                check(lib.htrvt_stem_stats(ptr(img), ptr(stats), ptr(w1), ptr(part), ptr(cs), B, H, W, C1, u8, st), "stem_stats")
            bn = self.bn_coeffs(P, "patch_embed.bn1", C1, train, cs, 1, B * (H // 2) * W, save=save)
            check(lib.htrvt_stem_fwd(ptr(img), ptr(stats), ptr(w1), ptr(bn.scale), ptr(bn.shift), ptr(a), ptr(idx), B, H, W, C1,
                                     self.dti, u8, st), "stem_fwd")
        else:
            c1 = self._empty(B, H // 2, W, C1)
            cs = self._empty(B * (H // 2) + 64, 2, C1, dtype=torch.float32) if train else self._empty(B * (H // 2), 2, C1, dtype=torch.float32)
            check(lib.htrvt_conv1_fwd(ptr(img), ptr(stats), ptr(w1), ptr(c1), ptr(cs), B, H, W, C1, self.dti, u8, st), "conv1_fwd")
            bn = self.bn_coeffs(P, "patch_embed.bn1", C1, train, cs, B * (H // 2), B * (H // 2) * W, save=save)
            check(lib.htrvt_bn_relu_maxpool(ptr(c1), ptr(bn.scale), ptr(bn.shift), ptr(a), ptr(idx), B, H // 2, W, C1, self.dti, st),
                  "bn_relu_maxpool")
        if save:
            sv.update(img=img, stats=stats, c1=c1, bn1=bn, idx=idx, c1_shape=(B, H // 2, W, C1))
        return a

    def _res_block_geoms(self, b, x):
        """ConvGeoms of the block `b` (StemBlock) on the input x: (conv1, conv2, downsample or None)"""
        B, Hc, Wc, _ = x.shape
        g1 = ConvGeom(B, Hc, Wc, b.Cin, b.planes, 3, b.stride, 1)
        g2 = ConvGeom(B, g1.Ho, g1.Wo, b.planes, b.planes, 3, (1, 1), 1)
        return g1, g2, ConvGeom(B, Hc, Wc, b.Cin, b.planes, 1, b.stride, 0) if b.downsample else None

    def _res_block_fwd_eval(self, P, b, x, train=False, save=False):
        """one residual block, not train and not save: running statistics are known up front, every BatchNorm (+ residual +
        ReLU) rides in the epilogue of its convolution: 2-3 launches per block, no normalisation passes.  (out, None)"""
        p = b.prefix
        g1, g2, gd = self._res_block_geoms(b, x)
        wf1, _ = self._conv_w(p + ".conv1", P[p + ".conv1.weight"])
        wf2, _ = self._conv_w(p + ".conv2", P[p + ".conv2.weight"])
        a1, _, _ = self.conv_fwd(x, wf1, g1, False, bn=self.bn_coeffs(P, p + ".bn1", b.planes, False), relu=True)
        bn_b = self.bn_coeffs(P, p + ".bn2", b.planes, False)
        res = x
        if gd is not None:
            wfd, _ = self._conv_w(p + ".downsample.0", P[p + ".downsample.0.weight"])
            res, _, _ = self.conv_fwd(x, wfd, gd, False, bn=self.bn_coeffs(P, p + ".downsample.1", b.planes, False))
        out, _, _ = self.conv_fwd(a1, wf2, g2, False, bn=bn_b, relu=True, residual=res)
        return out, None

    def _conv_bn(self, P, x, wf, g, prefix, train, save):
        """raw convolution + the coefficients of the BatchNorm behind it (train: batch statistics from the conv's epilogue)"""
        c, cs, rows = self.conv_fwd(x, wf, g, train)
        return SavedBN(self.bn_coeffs(P, prefix, g.Co, train, cs, rows, g.B * g.Ho * g.Wo, save=save), prefix, c)

    def _res_block_fwd(self, P, b, x, train, save):
        """one residual block with separate BatchNorm passes (train mode, or an eval forward that saves for its backward):
        (out, ResBlockSaved or None)"""
        p = b.prefix
        g1, g2, gd = self._res_block_geoms(b, x)
        wf1, _ = self._conv_w(p + ".conv1", P[p + ".conv1.weight"])
        wf2, _ = self._conv_w(p + ".conv2", P[p + ".conv2.weight"])
        bn_a = self._conv_bn(P, x, wf1, g1, p + ".bn1", train, save)
        a1 = self.bn_apply(bn_a.x, bn_a.coef.scale, bn_a.coef.shift, relu=True)
        bn_b = self._conv_bn(P, a1, wf2, g2, p + ".bn2", train, save)
        if gd is not None:
            wfd, _ = self._conv_w(p + ".downsample.0", P[p + ".downsample.0.weight"])
            bn_d = self._conv_bn(P, x, wfd, gd, p + ".downsample.1", train, save)
            res_kw = dict(res=bn_d.x, rscale=bn_d.coef.scale, rshift=bn_d.coef.shift)
        else:
            bn_d, res_kw = None, dict(res=x)
        # the block's output ReLU: the forward BatchNorm pass writes its 1-bit mask, and its backward (fused into the
        # NEXT block's conv1 dgrad) reads that instead of the activation
        want_mask = bool(save and self.fuse_bn_backward and self.dtype == torch.bfloat16 and b.planes % 8 == 0)
        out = self.bn_apply(bn_b.x, bn_b.coef.scale, bn_b.coef.shift, relu=True, want_mask=want_mask, **res_kw)
        out, omask = out if want_mask else (out, None)
        return out, (ResBlockSaved(p, x, g1, bn_a, a1, g2, bn_b, gd, bn_d, out, omask) if save else None)

    def _tokens_fwd(self, P, x, keep, B, Hc, Wc, sv):
        """final maxpool + span mask + pos-embed -> tokens (resnet18.py:82, HTR_VT.py:226-231): (tok [B,N,D], N)"""
        s, st = self.s, stream()
        Ht = (Hc - 1) // 2 + 1
        N = Ht * Wc
        assert N == s.num_patches, f"token count {N} != num_patches {s.num_patches}"
        D = s.D
        tok = self._empty(B, N, D)
        if s.pos_table is not None:     # LGP fork: the model's own table (no state-dict entry)
            if self._pos_table is None:
                self._pos_table = s.pos_table.to(self.dev).contiguous()
            pos = self._pos_table
        elif s.pos_embed:
            pos = P["pos_embed"].reshape(N, D)
        else:                       # window fork: no absolute position embedding (HTR_VT.py:265 of model_window)
            if self._zero_pos is None or self._zero_pos.shape != (N, D):
                self._zero_pos = torch.zeros(N, D, dtype=torch.float32, device=self.dev)
            pos = self._zero_pos
        if keep is not None and keep.dim() == 2:    # [B, N]: one mask row per sample
            check(lib.htrvt_pool_tokens_ps(ptr(x), ptr(keep), N, ptr(P["mask_token"]), ptr(pos), ptr(tok), B, Hc, N, D,
                                           self.dti, st), "pool_tokens_ps")
        else:
            check(lib.htrvt_pool_tokens(ptr(x), ptr(keep), ptr(P["mask_token"]), ptr(pos), ptr(tok), B, Hc, N, D, self.dti, st),
                  "pool_tokens")
        if sv is not None:
            sv["l3"], sv["keep"], sv["l3_shape"] = x, keep, (B, Hc, Wc)
        return tok, N

    def _encoder_fwd(self, P, xt, B, N, save):
        """transformer blocks (HTR_VT.py:80-83), each through the forward of its kind: (output, what the backwards keep)"""
        enc_saved = []
        for i, (kind, arg) in enumerate(self.s.blocks):
            e, xt = self._BLOCK[kind][0](self, P, f"blocks.{i}", kind, arg, xt, B, N, save)
            enc_saved.append(e)
        return xt, enc_saved

    def _head_fwd(self, P, xt, B, N, train, sv, want_features):
        """norm + head + sequence LayerNorm (HTR_VT.py:236-239): (logits, feature tap or None)"""
        s, st = self.s, stream()
        M, D, save = B * N, s.D, sv is not None
        xn, mn, rn = self.ln_fwd(P, "norm", xt, save)
        wh, _ = self._head_w(P["head.weight"])
        raw = self._empty(M, s.nb_cls, dtype=torch.float32)
        gemm(xn, wh, raw, dtype=self.dtype, M=M, N=s.nb_cls, K=D, lda=D, ldb=D, ldc=s.nb_cls, bias=P["head.bias"], c_f32=True)
        if s.whiten_logits:
            y = self._empty(B, N, s.nb_cls, dtype=torch.float32)
            sstats = self._empty(B, 2, dtype=torch.float32)
            check(lib.htrvt_seq_whiten_fwd(ptr(raw), ptr(y), ptr(sstats), B, N * s.nb_cls, WHITEN_EPS, 0, st), "seq_whiten_fwd")
        else:                       # window fork: head(norm(x)) is the output (no LayerNorm of the logits)
            y, sstats = raw.view(B, N, s.nb_cls), None
        if save:
            sv.update(x_last=xt, xn=xn, mn=mn, rn=rn, y=y, sstats=sstats, B=B, N=N, train=train)
        feats = None
        if want_features:       # a copy: xn is kept for the head's weight gradient and must not be written by the caller
            feats = torch.empty(B, N, D, dtype=torch.float32, device=self.dev)
            check(lib.htrvt_sgm_convert(ptr(xn), self.dti, ptr(feats), 0, M * D, 0, st), "sgm_convert")
        return y, feats

    # ------------------------------------------------------------------ a Linear's launch sequences, said once
    def _lin_fwd(self, P, name, x, act=0, preact=None, residual=None, out=None):
        """y = act(x @ W^T + b) [+ residual] of the Linear `name`"""
        w, _ = self._lin_w(name, P[name + ".weight"])
        return self.linear_fwd(x, w, P[name + ".bias"], out=out, act=act, preact=preact, residual=residual)

    def _lin_bwd(self, P, G, name, dy, x, act=0, preact=None, cols=None):
        """backward of the Linear `name` with input x: returns dx (optionally * gelu'(preact)); the weight and bias gradients
        go into G on the weight-gradient stream.  cols = (first, N): dy is that column block of a wider tensor."""
        w, wt = self._lin_w(name, P[name + ".weight"])
        dx = self.linear_dgrad(dy, w, wt, act=act, preact=preact, cols=cols)
        self.linear_wgrad(dy, x, G[name + ".weight"], G[name + ".bias"], cols=cols)
        return dx

    # ------------------------------------------------------------------ attention: the qkv Linear + the scores of one kind
    def _attn_fwd(self, P, pa, kind, arg, x, B, N, save):
        """the attention module `pa` up to its projection: qkv = Linear(x), then attention of `kind` over N tokens per image.
        Returns (qkv, O, (P, lse)): the probabilities or the log-sum-exp, whichever the route's backward reads, else None."""
        s = self.s
        h = s.heads
        qkv = self._lin_fwd(P, pa + ".qkv", x)
        if kind == "local":     # inside windows of arg = (window, shift) (csrc/lgp.hip; padding slots = the qkv bias, no mask
            # across the wrap): nothing but qkv and O is kept, the backward recomputes the windows' softmax
            return qkv, seq_ops.local_attention_fwd(qkv, P[pa + ".qkv.bias"], B, N, h, *arg), (None, None)
        bias = None
        if kind == "relpos":    # the block's relative-position table, arg = (window, shift), on the scores
            tab, tp = P[pa + ".relative_position_bias_table"], s.table_patches
            if self.dtype == torch.bfloat16:    # the table-driven fused kernels (csrc/attn_relpos.hip)
                if not lib.htrvt_attn_relpos_supported(N, s.hd, self.dti, tp, *arg):
                    raise RuntimeError(f"{pa}: relative-position attention: {lib.htrvt_last_error().decode()}")
                O, lse = seq_ops.relpos_attention_fwd(qkv, tab, B, N, h, tp, *arg, save=save)
                return qkv, O, (None, lse)
            assert not self.split, "split_bf16: no relative-position attention"
            bias = seq_ops.relpos_bias_fwd(tab, N, tp, *arg, N)     # float32: a dense bias into the batched-GEMM route
        elif self.fused_attention and lib.htrvt_attn_supported(N, s.hd, self.dti):
            # bf16: one launch, scores / probabilities stay on chip; lse is what the recomputing backward needs
            O, lse = seq_ops.attention_fwd(qkv, B, N, h, save=save)
            return qkv, O, (None, lse)
        O, Pm = seq_ops.attention_unfused_fwd(qkv, B, N, h, bias=bias)
        return qkv, O, (Pm, None)

    def _attn_bwd(self, P, G, pa, kind, arg, x, qkv, O, kept, dO, B, N):
        """backward of _attn_fwd: the gradient of x.  The qkv Linear's gradients and the relative-position table's are ADDED
        to G (every route is reproducible: fixed-order sums, no atomics)."""
        s = self.s
        h = s.heads
        Pm, lse = kept
        if kind == "local":
            dqkv, dpad = seq_ops.local_attention_bwd(qkv, P[pa + ".qkv.bias"], dO, B, N, h, *arg)
        elif kind == "relpos":
            name, tp = pa + ".relative_position_bias_table", s.table_patches
            gt = G.get(name)
            if Pm is None:
                dqkv = seq_ops.relpos_attention_bwd(qkv, P[name], O, dO, lse, B, N, h, tp, *arg, dtable=gt)
            else:
                dbias = torch.zeros(h, N, N, dtype=torch.float32, device=self.dev)
                dqkv = seq_ops.attention_unfused_bwd(qkv, Pm, dO, B, N, h, dbias=dbias)
                if gt is not None:
                    dtab = seq_ops.relpos_bias_bwd(dbias, N, tp, *arg)
                    check(lib.htrvt_rowsum_f32(ptr(dtab), 1, dtab.numel(), ptr(gt), stream()), "rowsum")
        elif Pm is None:        # fused forward: recomputing fused backward (dQ launch, then dK/dV launch)
            dqkv = seq_ops.attention_bwd(qkv, O, dO, lse, B, N, h)
        else:
            dqkv = seq_ops.attention_unfused_bwd(qkv, Pm, dO, B, N, h)
        dx = self._lin_bwd(P, G, pa + ".qkv", dqkv, x)
        if kind == "local" and N % arg[0]:
            # ragged last window: its padding slots hold the qkv bias, so their k / v gradient belongs to the k / v thirds of
            # the bias gradient; on the weight-gradient stream, behind the bias column sum of the Linear above
            D, gb = s.D, G[pa + ".qkv.bias"]
            self._on_side(lambda: ops.colsum(dpad, B, 2 * D, 2 * D, gb.data_ptr() + 4 * D, dti=0), dpad)
        return dx

    # ------------------------------------------------------------------ the blocks, one forward / backward pair per kind
    def _mlp_fwd(self, P, p, x1, save):
        """x2 = x1 + fc2(gelu(fc1(norm2(x1)))); returns (x2, what the backward keeps)"""
        ln2, m2, r2 = self.ln_fwd(P, p + ".norm2", x1, save)
        hpre = self._empty(x1.shape[0], self.s.hidden) if save else None
        hact = self._lin_fwd(P, p + ".mlp.fc1", ln2, act=1, preact=hpre)
        x2 = self._lin_fwd(P, p + ".mlp.fc2", hact, residual=x1)
        return x2, dict(ln2=ln2, m2=m2, r2=r2, hpre=hpre, h=hact)

    def _mlp_bwd(self, P, G, e, dx):
        """gradient of the block's x1 (MLP branch + residual) from the gradient of its output"""
        p = e["p"]
        dhpre = self._lin_bwd(P, G, p + ".mlp.fc2", dx, e["h"], act=2, preact=e["hpre"])
        dln2 = self._lin_bwd(P, G, p + ".mlp.fc1", dhpre, e["ln2"])
        del dhpre
        return self.ln_bwd(P, G, p + ".norm2", dln2, e["x1"], e["m2"], e["r2"], dx)

    def _v1_block_fwd(self, P, p, kind, arg, xt, B, N, save):
        """the v1-shaped block (HTR_VT.py:27-39) with the attention of `kind` ("full", "relpos" or "local"):
        x1 = x + proj(attention(norm1(x))); x2 = x1 + mlp(norm2(x1)).  Returns (what the backward keeps or None, x2)."""
        ln1, m1, r1 = self.ln_fwd(P, p + ".norm1", xt, save)
        qkv, O, kept = self._attn_fwd(P, p + ".attn", kind, arg, ln1, B, N, save)
        x1 = self._lin_fwd(P, p + ".attn.proj", O, residual=xt)
        x2, mlp = self._mlp_fwd(P, p, x1, save)
        e = dict(kind=kind, arg=arg, p=p, x0=xt, ln1=ln1, m1=m1, r1=r1, qkv=qkv, O=O, attn=kept, x1=x1, **mlp) if save else None
        return e, x2

    def _v1_block_bwd(self, P, G, e, dx, B, N):
        p = e["p"]
        dx1 = self._mlp_bwd(P, G, e, dx)                                  # MLP: x2 = x1 + fc2(gelu(fc1(ln2)))
        dO = self._lin_bwd(P, G, p + ".attn.proj", dx1, e["O"])           # attention: x1 = x0 + proj(attn(ln1))
        dln1 = self._attn_bwd(P, G, p + ".attn", e["kind"], e["arg"], e["ln1"], e["qkv"], e["O"], e["attn"], dO, B, N)
        return self.ln_bwd(P, G, p + ".norm1", dln1, e["x0"], e["m1"], e["r1"], dx1)

    def _lgp_block_fwd(self, P, p, kind, arg, xt, B, N, save):
        """the LGP fork's block (model_lgp/model/plg.py:172-212): x1 = x + fuse([local_attn(y) | global_attn(y)]), y = norm1(x);
        x2 = x1 + mlp(norm2(x1)).  The two branches write the halves of one [B N][2D] buffer (no cat copy); csrc/lgp.hip has
        the window attention, the pooling + LayerNorm in front of the global branch and the scaled up-sampling behind it,
        everything else is the kernels of the v1 block."""
        D, M = self.s.D, B * N
        win, gtok, beps = arg
        Gt = min(gtok, N)
        ln1, m1, r1 = self.ln_fwd(P, p + ".norm1", xt, save)
        cat = self._empty(M, 2 * D)
        # local branch: qkv -> attention inside windows (padding slots = the qkv bias) -> proj into the left half
        qkv, O, kept = self._attn_fwd(P, p + ".local_attn", "local", (win, 0), ln1, B, N, save)
        self._lin_fwd(P, p + ".local_attn.proj", O, out=cat[:, :D])
        # global branch: pool to Gt tokens + LayerNorm -> qkv -> full attention -> proj -> up-sample * sigmoid(alpha), right half
        z, _, zrstd = seq_ops.pool_norm_fwd(ln1, B, N, Gt, beps)
        qkvg, Og, keptg = self._attn_fwd(P, p + ".global_attn", "full", None, z, B, Gt, save)
        yg = self._lin_fwd(P, p + ".global_attn.proj", Og)
        seq_ops.upsample_fwd(yg, P[p + ".global_attn.logit_alpha"], cat[:, D:], B, N, Gt)
        x1 = self._lin_fwd(P, p + ".fuse", cat, residual=xt)
        x2, mlp = self._mlp_fwd(P, p, x1, save)
        e = dict(kind=kind, p=p, x0=xt, ln1=ln1, m1=m1, r1=r1, qkv=qkv, O=O, attn=kept, cat=cat, z=z, zrstd=zrstd, qkvg=qkvg,
                 attng=keptg, Og=Og, yg=yg, x1=x1, win=win, Gt=Gt, **mlp) if save else None
        return e, x2

    def _lgp_block_bwd(self, P, G, e, dx, B, N):
        D, p, win, Gt = self.s.D, e["p"], e["win"], e["Gt"]
        dx1 = self._mlp_bwd(P, G, e, dx)
        dcat = self._lin_bwd(P, G, p + ".fuse", dx1, e["cat"])       # [M][2D]: left half d local proj, right half d global
        # global branch
        dyg = seq_ops.upsample_bwd(dcat[:, D:], e["yg"], P[p + ".global_attn.logit_alpha"], G[p + ".global_attn.logit_alpha"],
                                   B, N, Gt)
        dOg = self._lin_bwd(P, G, p + ".global_attn.proj", dyg, e["Og"])
        dz = self._attn_bwd(P, G, p + ".global_attn", "full", None, e["z"], e["qkvg"], e["Og"], e["attng"], dOg, B, Gt)
        # local branch
        dO = self._lin_bwd(P, G, p + ".local_attn.proj", dcat, e["O"], cols=(0, D))
        dln1 = self._attn_bwd(P, G, p + ".local_attn", "local", (win, 0), e["ln1"], e["qkv"], e["O"], e["attn"], dO, B, N)
        seq_ops.pool_norm_bwd(dz, e["z"], e["zrstd"], B, N, Gt, dx=dln1)      # added to the local branch's gradient
        return self.ln_bwd(P, G, p + ".norm1", dln1, e["x0"], e["m1"], e["r1"], dx1)

    # block kind -> (forward, backward); ModelShape.blocks says which kind each block is
    _BLOCK = {"full": (_v1_block_fwd, _v1_block_bwd), "relpos": (_v1_block_fwd, _v1_block_bwd),
              "local": (_v1_block_fwd, _v1_block_bwd), "lgp": (_lgp_block_fwd, _lgp_block_bwd)}

    # ------------------------------------------------------------------ backward
    def backward(self, P, G, dy, after_encoder=None, after_layer3=None, dfeats=None):
        """dy: float32 [B,N,C] = dLoss/dlogits (None: only the features carry a loss).  dfeats: None or float32 [B,N,D] =
        dLoss/dfeats of forward(want_features=True), added to the final norm's output gradient.  Accumulates dLoss/dparam
        into G (dict name -> float32 tensor, same shapes as P; the caller zeroes it).  Uses the activations saved by
        forward(save=True)."""
        sv = self.saved
        assert sv is not None, "backward() needs forward(..., save=True)"
        s, st = self.s, stream()
        B, N, D, C = sv["B"], sv["N"], s.D, s.nb_cls
        M = B * N
        assert dy is not None or dfeats is not None, "backward() needs dy and / or dfeats"
        if dfeats is not None:
            dfeats = dfeats.contiguous()
            assert dfeats.dtype == torch.float32 and dfeats.shape == (B, N, D) and not self.split
        self._zarena_begin()
        self._pending_unpack = []
        self._bn_train = bool(sv["train"])
        self._side_active = self.overlap_wgrad and not self.single_stream
        if dy is None:          # features-only loss: the head and the logits' LayerNorm get no gradient
            dxn = self._empty(M, D)
            check(lib.htrvt_sgm_convert(ptr(dfeats), 0, ptr(dxn), self.dti, M * D, 0, st), "sgm_convert")
        else:
            dxn = self._head_backward(P, G, sv, dy.contiguous(), B, N, M, C, D, st)
            if dfeats is not None:
                check(lib.htrvt_sgm_convert(ptr(dfeats), 0, ptr(dxn), self.dti, M * D, 1, st), "sgm_convert")
        dx = self._encoder_bwd(P, G, sv, dxn, B, N, after_encoder)
        dfeat = self._tokens_bwd(G, sv, dx, B, N)
        self._stem_bwd(P, G, sv, dfeat, B, after_layer3)
        self._flush_unpacks()
        self._join_side()
        self._side_active = False
        self._zarena_end()
        self._split_cache = []
        self._saved_planes = {}
        self.saved = None

    def _head_backward(self, P, G, sv, dy, B, N, M, C, D, st):
        s = self.s
        assert dy.dtype == torch.float32 and dy.shape == (B, N, C)
        # sequence LN, head, final norm
        Cp = (C + 7) // 8 * 8           # class dim padded so that every 16-byte chunk is aligned
        if s.whiten_logits:
            draw = torch.zeros(M, Cp, dtype=self.dtype, device=self.dev)
            check(lib.htrvt_seq_whiten_bwd(ptr(dy), ptr(sv["y"]), ptr(sv["sstats"]), ptr(draw), B, N, C, Cp, self.dti, st),
                  "seq_whiten_bwd")
        elif Cp == C and self.dtype == torch.float32:    # window fork: the gradient of the raw logits is dy itself
            draw = dy.view(M, C)
        elif Cp == C:
            draw = self._empty(M, C)
            check(lib.htrvt_cast_f32(ptr(dy), ptr(draw), M * C, self.dti, st), "cast_f32")
        else:
            draw = torch.zeros(M, Cp, dtype=self.dtype, device=self.dev)
            draw[:, :C].copy_(dy.view(M, C))
        wh, wht = self._head_w(P["head.weight"])
        dxn = self.linear_dgrad(draw, wh, wht, plain=True)      # (split mode: the 80-class head stays on the float32 kernels)
        if Cp == C:
            self.linear_wgrad(draw, sv["xn"], G["head.weight"], G["head.bias"], plain=True)
        else:
            dwp, dbp = self._zeros(Cp, D), self._zeros(Cp)
            self.linear_wgrad(draw, sv["xn"], dwp, dbp, plain=True)
            self._join_side()
            check(lib.htrvt_rowsum_f32(ptr(dwp), 1, C * D, ptr(G["head.weight"]), st), "rowsum")
            check(lib.htrvt_rowsum_f32(ptr(dbp), 1, C, ptr(G["head.bias"]), st), "rowsum")
        return dxn

    def _encoder_bwd(self, P, G, sv, dxn, B, N, after_encoder):
        """final norm and the encoder blocks, last to first, each through the backward of its kind: the gradient of the tokens"""
        dx = self.ln_bwd(P, G, "norm", dxn, sv["x_last"], sv["mn"], sv["rn"], None)
        for e in reversed(sv["enc"]):
            dx = self._BLOCK[e["kind"]][1](self, P, G, e, dx, B, N)
        if after_encoder is not None:   # every blocks.*, norm, head gradient is enqueued: DP bucket can go
            after_encoder(self._wgrad_stream())      # (the collective waits for the weight-gradient stream, not this one)
        return dx

    def _tokens_bwd(self, G, sv, dx, B, N):
        """token assembly: the mask token's gradient and the gradient of the layer-3 output"""
        st, M, D = stream(), B * N, self.s.D
        keep = sv["keep"]
        per_sample = keep is not None and keep.dim() == 2
        if keep is not None:        # a [B, N] mask is one flag per token row: keep_mod = B N
            ops.colsum(dx, M, D, D, G["mask_token"], dti=self.dti, keep=keep, keep_mod=M if per_sample else N)
        Bq, Hc, Wc = sv["l3_shape"]
        dfeat = self._empty(Bq, Hc, Wc, D)
        if per_sample:
            check(lib.htrvt_pool_tokens_bwd_ps(ptr(dx), ptr(sv["l3"]), ptr(keep), N, ptr(dfeat), B, Hc, N, D, self.dti, st),
                  "pool_tokens_bwd_ps")
        else:
            check(lib.htrvt_pool_tokens_bwd(ptr(dx), ptr(sv["l3"]), ptr(keep), ptr(dfeat), B, Hc, N, D, self.dti, st),
                  "pool_tokens_bwd")
        return dfeat

    def _stem_bwd(self, P, G, sv, dfeat, B, after_layer3):
        """residual stages, last block to first, then the first max-pool + bn1 + conv1"""
        blocks = sv["stem_blocks"]
        hook_at = max(i for i, blk in enumerate(blocks) if not blk.p.startswith("patch_embed.layer3."))
        grad = StemGrad(dfeat)      # from the token kernel: a raw gradient
        for i in reversed(range(len(blocks))):
            if i == hook_at and after_layer3 is not None:     # layer 3 (78 % of the stem's weights) is done: its DP bucket can go
                self._flush_unpacks()
                after_layer3(self._wgrad_stream())
            grad = self._res_block_bwd(P, G, blocks[i], blocks[i - 1] if i > 0 else None, grad)
        self._stem_head_bwd(P, G, sv, grad.g, B)

    def can_fuse(self, g):
        """the dgrad of `g` runs on the LDS-DMA kernel (bf16, > 128 rows per launch): its epilogue can mask and take BN sums"""
        return (self.fuse_bn_backward and self.dtype == torch.bfloat16 and
                g.B * g.Hi * g.Wi // (g.sh * g.sw) > 128 and g.Ci % 8 == 0)

    def _res_block_bwd(self, P, G, blk, prev, grad):
        """backward of one residual block from the StemGrad of its output: the StemGrad of `prev`, the block in front of it
        (None: the stem head).  bf16: the ReLU mask of a block's output and the BatchNorm-backward sums of its bn2 (and
        downsample BN) come from the epilogue of the dgrad GEMM that creates that gradient; float32 keeps the separate pass."""
        p, bn_a, bn_b, bn_d = blk.p, blk.bn_a, blk.bn_b, blk.bn_d
        # downsample gradient as one more tap of the strided conv's class-(0,0) dgrad (HtrvtGemmDesc.A2) instead of its own
        # parity-class launches plus a residual round trip of the whole input gradient: d(conv1 out) and d(downsample
        # out) then live back to back in one allocation (the second gather source sits at a fixed offset from the first)
        fuse_ds = (not self.split and blk.gd is not None and self._dgrad_by_class(blk.g1) and
                   2 * bn_a.x.numel() * bn_a.x.element_size() < 2 ** 31 - 64)     # A2 lies behind A inside ONE 2 GiB descriptor
        # --- 1. BatchNorm backward of the block's output: dcb = d(conv2 out), gm = dOut * (out > 0) [, dcd = d(downsample out)]
        if grad.sums is None:      # raw gradient: mask + sums in one reduction pass, then the apply
            dcb, gm = self.bn_backward(grad.g, blk.out, bn_b, P, G, want_g=True)
            sums_b = sums_d = None
        else:                      # the sums are taken out of the record: their buffers die with this call's references
            gm, sums_b, sums_d = grad.g, grad.sums.pop(0), (grad.sums.pop(0) if grad.sums else None)
        pair = self._empty(2, *bn_a.x.shape) if fuse_ds else None     # (behind the unfused reduce's own buffers)
        dca_out, dcd_out, dcd = (pair[0], pair[1], None) if fuse_ds else (None, None, None)
        if sums_d is not None and self.merge_bn_backward:
            # bn2 and the downsample BN take the same gradient: one pass, gm read once (csrc/bwd.hip bn_bwd_apply2)
            co_b = self.bn_backward_coef(*sums_b, bn_b, P, G)
            co_d = self.bn_backward_coef(*sums_d, bn_d, P, G)
            dcb = torch.empty_like(bn_b.x)
            dcd = dcd_out if fuse_ds else torch.empty_like(bn_d.x)
            C = bn_b.x.shape[-1]
            check(lib.htrvt_bn_bwd_apply2(ptr(gm), ptr(bn_b.x), ptr(co_b), ptr(dcb), ptr(bn_d.x), ptr(co_d), ptr(dcd),
                                          dcb.numel() // C, C, self.dti, stream()), "bn_bwd_apply2")
        elif sums_b is not None:
            dcb, _ = self.bn_backward_finish(*sums_b, gm, None, bn_b, P, G)
        del sums_b
        # --- 2. conv2: weight gradient, dgrad, bn1 backward: dca = d(conv1 out)
        dca = self._conv2_bwd(P, G, blk, dcb, dca_out)
        del dcb
        # --- 3. conv1 [+ downsample]: weight gradient(s), then the dgrad(s) with what they feed folded into the epilogue
        _, wd1 = self._conv_w(p + ".conv1", P[p + ".conv1.weight"])
        self.conv_wgrad(dca, blk.x, blk.g1, G[p + ".conv1.weight"])
        kw, sums = {}, None      # the gradient of this block's INPUT feeds prev's output: ReLU + bn2 [+ downsample BN]
        if prev is not None and self.can_fuse(blk.g1):
            bns = [prev.bn_b] + ([prev.bn_d] if prev.gd is not None else [])
            bnb, sums = self._bnb_request(bns, self.dgrad_tiles(blk.g1))
            kw = dict(relu_src=prev.out, bnb=bnb)
            # the bit-mask form is compiled for (one sum set) and (residual + one or two sets); fuse_ds: no residual
            if prev.mask is not None and (len(bns) == 1 or not fuse_ds):
                kw.update(relu_src=prev.mask, relu_bits=True)
        if blk.gd is None:
            return StemGrad(self.conv_dgrad(dca, wd1, blk.g1, residual=gm, **kw), sums)
        if dcd is None and sums_d is not None:      # (else it came out of the joint pass with bn2 above)
            dcd, _ = self.bn_backward_finish(*sums_d, gm, None, bn_d, P, G, out=dcd_out)
        elif dcd is None:
            dcd, _ = self.bn_backward(gm, None, bn_d, P, G, out=dcd_out)
        _, wdd = self._conv_w(p + ".downsample.0", P[p + ".downsample.0.weight"])
        self.conv_wgrad(dcd, blk.x, blk.gd, G[p + ".downsample.0.weight"])
        if fuse_ds:
            wdj = self._conv_w_joint_dgrad(p + ".conv1", P[p + ".conv1.weight"], p + ".downsample.0", P[p + ".downsample.0.weight"])
            return StemGrad(self.conv_dgrad(dca, wdj, blk.g1, extra=dcd, **kw), sums)
        dres = self.conv_dgrad(dcd, wdd, blk.gd)
        return StemGrad(self.conv_dgrad(dca, wd1, blk.g1, residual=dres, **kw), sums)

    def _conv2_bwd(self, P, G, blk, dcb, out):
        """conv2's weight gradient and dgrad, then bn1's backward (written into `out` when given): d(conv1 out)"""
        p, bn_a = blk.p, blk.bn_a
        _, wd2 = self._conv_w(p + ".conv2", P[p + ".conv2.weight"])
        self.conv_wgrad(dcb, blk.a1, blk.g2, G[p + ".conv2.weight"])
        if not self.can_fuse(blk.g2):
            da1 = self.conv_dgrad(dcb, wd2, blk.g2)
            return self.bn_backward(da1, blk.a1, bn_a, P, G, out=out)[0]
        bnb, sums = self._bnb_request([bn_a], self.dgrad_tiles(blk.g2))
        # a1 = relu(bn1(ca)): the mask is recomputed from ca (read for the sums anyway) instead of reading a1
        rk = dict(relu_bn=(bn_a.coef.scale, bn_a.coef.shift)) if self.relu_mask_from_bn else dict(relu_src=blk.a1)
        g1 = self.conv_dgrad(dcb, wd2, blk.g2, bnb=bnb, **rk)
        return self.bn_backward_finish(*sums[0], g1, None, bn_a, P, G, out=out)[0]

    def _stem_head_bwd(self, P, G, sv, dout, B):
        """the first max-pool + bn1 + conv1 (Cin = 1) from the gradient of the pooled activations"""
        st = stream()
        img, c1, bn = sv["img"], sv["c1"], sv["bn1"]
        u8 = 1 if img.dtype == torch.uint8 else 0
        _, Hh, W, C1 = sv["c1_shape"]
        if self.fuse_conv1_backward and self._bn_train:
            # dW1, dgamma, dbeta from per-channel sums over the pooled gradient (csrc/conv1_bwd.hip)
            partial = self._empty(lib.htrvt_conv1_bwd_rows(B, 2 * Hh), lib.htrvt_conv1_bwd_row_floats(C1), dtype=torch.float32)
            check(lib.htrvt_conv1_bwd(ptr(img), ptr(sv["stats"]), ptr(dout), ptr(sv["idx"]), ptr(P["patch_embed.conv1.weight"]),
                                      ptr(P["patch_embed.bn1.weight"]), ptr(bn.mean), ptr(bn.rstd), ptr(partial),
                                      ptr(G["patch_embed.conv1.weight"]), ptr(G["patch_embed.bn1.weight"]),
                                      ptr(G["patch_embed.bn1.bias"]), B, 2 * Hh, W, C1, self.dti, u8, st), "conv1_bwd")
            return
        g = torch.empty_like(c1)
        check(lib.htrvt_maxpool_bwd(ptr(dout), ptr(sv["idx"]), ptr(c1), ptr(bn.scale), ptr(bn.shift), ptr(g), B, Hh, W, C1,
                                    self.dti, st), "maxpool_bwd")
        dc1, _ = self.bn_backward(g, None, SavedBN(bn, "patch_embed.bn1", c1), P, G)
        del g
        partial = self._empty(lib.htrvt_conv1_wgrad_blocks(B, 2 * Hh), C1 * 9, dtype=torch.float32)
        check(lib.htrvt_conv1_wgrad(ptr(img), ptr(sv["stats"]), ptr(dc1), ptr(G["patch_embed.conv1.weight"]), ptr(partial),
                                    B, 2 * Hh, W, C1, self.dti, u8, st), "conv1_wgrad")
