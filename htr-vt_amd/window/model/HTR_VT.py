"""MI355X-native window-attention HTR-VT behind the fork's Python API.

Drop-in for model_window/model/HTR_VT.py:
    create_model(nb_cls, img_size, **kwargs) -> nn.Module
    module(x, mask_ratio=0.0, max_span_length=1, use_masking=False) -> raw logits [B, N, nb_cls] (head(norm(x)), no
    LayerNorm of the logits)
Same module tree, names and construction order as the fork (HTR_VT.py:233-276): no pos_embed; every block owns
`attn.relative_position_bias_table` [2P-1, heads] (zeros) and the persistent int64 `attn.relative_position_index`
buffer; blocks 0 / 1 attend in 1-D windows of 16 tokens (shift 0 / 8), blocks 2 / 3 attend fully, all with the bias.
`torch.manual_seed(s); create_model(...)` gives the fork's initial state_dict, including what its constructor's zero-image
pass through the stem leaves in every BatchNorm (running_var 0.9, num_batches_tracked 1) -- restated here without running
the stem.  P (the table size) is the token count of that pass, which runs the image transposed ([1, 1, W, H]).

Dropout is not implemented: the fork hard-codes dropout 0.1 (proj / MLP), attention dropout 0.05 and drop-path up to 0.1.
They are identity in eval mode, so evaluation and inference run as in the fork; a train-mode forward raises
NotImplementedError unless the model was built with `create_model(..., dropout=False)` (an addition of this drop-in),
which trains the same network without them.
"""
from functools import partial

import torch
import torch.nn as nn

try:                                    # `from model import HTR_VT` (fork layout, htr-vt_amd/window on sys.path)
    from model import resnet18
except ImportError:                     # `from htrvt_amd.window.model import HTR_VT`
    from . import resnet18

import htrvt_amd                        # noqa: F401  (loads libhtrvt_hip.so or raises)
from htrvt_amd.engine import ModelShape, stem_tokens
from htrvt_amd.model import HTR_VT as _V1

Mlp, LayerNorm, _no_eager = _V1.Mlp, _V1.LayerNorm, _V1._no_eager

WINDOWS = {0: (16, 0), 1: (16, 8)}      # block -> (window, shift); other blocks: full attention (HTR_VT.py:255-256)


class Attention(nn.Module):
    def __init__(self, dim, num_patches, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        assert dim % num_heads == 0, 'dim should be divisible by num_heads'
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.num_patches = num_patches
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * num_patches - 1), num_heads))
        coords = torch.arange(num_patches)
        self.register_buffer("relative_position_index", coords[None, :] - coords[:, None] + num_patches - 1)

    forward = _no_eager


class Block(nn.Module):
    def __init__(self, dim, num_heads, num_patches, mlp_ratio=4., qkv_bias=False, drop=0.0, attn_drop=0., drop_path=0.,
                 norm_layer=nn.LayerNorm, window_size=0, shift_size=0):
        super().__init__()
        self.window_size, self.shift_size, self.drop_path = window_size, shift_size, drop_path
        self.norm1 = norm_layer(dim, elementwise_affine=True)
        self.attn = Attention(dim, num_patches, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = norm_layer(dim, elementwise_affine=True)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    forward = _no_eager


class MaskedAutoencoderViT(_V1.MaskedAutoencoderViT):
    """HTR-VT encoder of the window fork; forward / span mask / engines as the model_v1 drop-in"""

    def __init__(self, nb_cls=80, img_size=[512, 32], patch_size=[8, 32], embed_dim=1024, depth=24, num_heads=16,
                 mlp_ratio=4., norm_layer=nn.LayerNorm, compute_dtype=torch.float32, dropout=True):
        nn.Module.__init__(self)
        if compute_dtype == "split_bf16":
            raise NotImplementedError("the window model has no split_bf16 path: use compute_dtype=torch.float32 (parity) "
                                      "or torch.bfloat16")
        self.layer_norm = LayerNorm()
        self.patch_embed = resnet18.ResNet18(embed_dim)
        self.grid_size = [img_size[0] // patch_size[0], img_size[1] // patch_size[1]]
        self.embed_dim = embed_dim
        # the fork counts the stem's output for a zero image [1, 1, img_size[1], img_size[0]] in train mode: that pass
        # leaves every BatchNorm with batch mean 0 / variance 0 folded in once (momentum 0.1)
        self.num_patches = stem_tokens(img_size[1], img_size[0])
        with torch.no_grad():
            for m in self.patch_embed.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.running_var.fill_(0.9)
                    m.num_batches_tracked.fill_(1)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        dpr = torch.linspace(0, 0.1, steps=depth).tolist()
        self.dropout = bool(dropout)
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, self.num_patches, mlp_ratio, qkv_bias=True, drop=0.1, attn_drop=0.05,
                  drop_path=dpr[i], norm_layer=norm_layer, window_size=WINDOWS.get(i, (0, 0))[0],
                  shift_size=WINDOWS.get(i, (0, 0))[1])
            for i in range(depth)])
        self.norm = norm_layer(embed_dim, elementwise_affine=True)
        self.head = torch.nn.Linear(embed_dim, nb_cls)
        self.initialize_weights()
        eps = {m.eps for m in self.modules() if isinstance(m, nn.LayerNorm)}
        assert len(eps) == 1, f"one LayerNorm eps per model expected, got {eps}"
        self.tokens = stem_tokens(img_size[0], img_size[1])     # tokens of a real [B, 1, H, W] image
        self._shape = ModelShape(nb_cls, img_size, embed_dim, depth, num_heads, mlp_ratio, patch_size, ln_eps=eps.pop(),
                                 pos_embed=False, whiten_logits=False,
                                 relpos=[(b.window_size, b.shift_size) for b in self.blocks],
                                 table_patches=self.num_patches, dropout=self.dropout)
        self.compute_dtype = compute_dtype
        self._engines = {}

    def initialize_weights(self):
        torch.nn.init.normal_(self.mask_token, std=.02)
        self.apply(self._init_weights)

    def forward(self, x, mask_ratio=0.0, max_span_length=1, use_masking=False, keep_mask=None):
        if self.training and self.dropout:
            raise NotImplementedError("train-mode forward with the fork's dropout / drop-path: not implemented; build the "
                                      "model with create_model(..., dropout=False) to train without them, or call eval()")
        if keep_mask is None and use_masking:      # the span mask covers the real tokens (HTR_VT.py:202-210 on x)
            keep_mask = self.generate_span_mask(self.tokens, mask_ratio, max_span_length)
        return super().forward(x, keep_mask=keep_mask)


def create_model(nb_cls, img_size, **kwargs):
    return MaskedAutoencoderViT(nb_cls, img_size=img_size, patch_size=(4, 64), embed_dim=768, depth=4, num_heads=6,
                                mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
