"""MI355X-native LGP (local-global parallel) HTR-VT behind the fork's Python API.

Drop-in for model_lgp/model/HTR_VT.py:
    create_model(nb_cls, img_size, **kwargs) -> nn.Module
    module(x, mask_ratio=0.0, max_span_length=1, use_masking=False) -> logits [B, N, nb_cls] (whitened, as model_v1)
Same module tree, names and construction order as the fork (HTR_VT.py:152-276, plg.py): every block is a
LocalGlobalParallelBlockSimple (window attention over 12 tokens beside attention over 64 pooled tokens, fused by a
Linear(2D, D)); `torch.manual_seed(s); create_model(...)` gives the fork's initial state_dict.  `pos_embed` is the
sin-cos table of the stem's real output grid [1, N], kept in a non-persistent buffer as in the fork: `model.pos_embed`
exists, `state_dict()` does not carry it (the fork builds it lazily at the first forward; here the grid is known from
img_size at construction).

The fork has no dropout and no drop-path, so train mode runs as it stands: its train.py / valid.py / test.py work
unchanged.  compute_dtype: torch.float32 (default, parity) or torch.bfloat16; "split_bf16" is not implemented."""
from functools import partial

import torch
import torch.nn as nn

try:                                    # `from model import HTR_VT` (fork layout, htr-vt_amd/lgp on sys.path)
    from model import resnet18
    from model.plg import LocalGlobalParallelBlockSimple
except ImportError:                     # `from htrvt_amd.lgp.model import HTR_VT`
    from . import resnet18
    from .plg import LocalGlobalParallelBlockSimple

import htrvt_amd                        # noqa: F401  (loads libhtrvt_hip.so or raises)
from htrvt_amd.engine import ModelShape, stem_tokens
from htrvt_amd.model import HTR_VT as _V1

Mlp, LayerNorm, _no_eager, get_2d_sincos_pos_embed = _V1.Mlp, _V1.LayerNorm, _V1._no_eager, _V1.get_2d_sincos_pos_embed

WINDOW = 12                             # HTR_VT.py:183


class Attention(nn.Module):
    """defined by the fork, built by nothing (HTR_VT.py:13-43)"""

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

    forward = _no_eager


class Block(nn.Module):
    """defined by the fork, built by nothing (HTR_VT.py:56-94)"""

    def __init__(self, dim, num_heads, num_patches, mlp_ratio=4., qkv_bias=False, drop=0.0, attn_drop=0., init_values=None,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim, elementwise_affine=True)
        self.attn = Attention(dim, num_patches, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = norm_layer(dim, elementwise_affine=True)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    forward = _no_eager


class MaskedAutoencoderViT(_V1.MaskedAutoencoderViT):
    """HTR-VT encoder of the LGP fork; forward / span mask / engines as the model_v1 drop-in"""

    def __init__(self, nb_cls=80, img_size=[512, 32], patch_size=[8, 32], embed_dim=1024, depth=3, num_heads=16,
                 mlp_ratio=4., norm_layer=nn.LayerNorm, compute_dtype=torch.float32):
        nn.Module.__init__(self)
        if compute_dtype == "split_bf16":
            raise NotImplementedError("the LGP model has no split_bf16 path: use compute_dtype=torch.float32 (parity) "
                                      "or torch.bfloat16")
        self.layer_norm = LayerNorm()
        self.patch_embed = resnet18.ResNet18(embed_dim)
        self.embed_dim = embed_dim
        self.grid_size = [img_size[0] // patch_size[0], img_size[1] // patch_size[1]]
        self.num_patches = self.grid_size[0] * self.grid_size[1]      # the fork's estimate, kept; the engine counts `tokens`
        self.mask_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        if img_size[0] != 64:      # the stem leaves H' = H / 64 rows; the table below is the fork's for H' = 1 only
            raise NotImplementedError(f"the LGP model is built for 64-pixel lines (img_size[0] = {img_size[0]}): the position "
                                      "table of a taller stem grid is not implemented")
        self.tokens = stem_tokens(img_size[0], img_size[1])           # [H', W'] = [1, tokens] for 64-pixel lines
        pe = torch.from_numpy(get_2d_sincos_pos_embed(embed_dim, (1, self.tokens))).float()
        self.register_buffer("pos_embed", pe.unsqueeze(0), persistent=False)
        self.blocks = nn.ModuleList([
            LocalGlobalParallelBlockSimple(dim=embed_dim, num_heads=num_heads, window_size=WINDOW, mlp_ratio=mlp_ratio,
                                           qkv_bias=True, drop=0.0, attn_drop=0.0, norm_layer=norm_layer, drop_path=0.0)
            for _ in range(depth)])
        self.norm = norm_layer(embed_dim, elementwise_affine=True)
        self.head = nn.Linear(embed_dim, nb_cls)
        self.initialize_weights()
        # the global branch's LayerNorm has no parameters and its own eps: the engine takes it per block, not per model
        eps = {m.eps for m in self.modules() if isinstance(m, nn.LayerNorm) and m.elementwise_affine}
        assert len(eps) == 1, f"one LayerNorm eps per model expected, got {eps}"
        g = self.blocks[0].global_attn
        assert all((b.local_attn.win, b.global_attn.g_tokens, b.global_attn.branch_norm.eps) ==
                   (WINDOW, g.g_tokens, g.branch_norm.eps) for b in self.blocks)
        self._shape = ModelShape(nb_cls, img_size, embed_dim, depth, num_heads, mlp_ratio, patch_size, ln_eps=eps.pop(),
                                 lgp=(WINDOW, g.g_tokens, g.branch_norm.eps), pos_table=pe.clone())
        self.compute_dtype = compute_dtype
        self._engines = {}
        self._pos_seen = self.pos_embed

    def _sync_pos_embed(self):
        """the engine adds the table it was built with; a caller who assigned `model.pos_embed` (the fork's buffer) gets
        that table used from the next forward (or Trainer construction) on"""
        pe = self.pos_embed
        if pe is getattr(self, "_pos_seen", None):
            return
        if pe is None or tuple(pe.shape) != (1, self.tokens, self.embed_dim):
            raise ValueError(f"pos_embed must be a [1, {self.tokens}, {self.embed_dim}] tensor, got "
                             f"{None if pe is None else tuple(pe.shape)}")
        self._shape.pos_table = pe.detach()[0].float().cpu().contiguous()
        for eng in self._engines.values():
            eng._pos_table = None
        self._pos_seen = pe

    def _engine(self, device):
        self._sync_pos_embed()
        return super()._engine(device)

    def initialize_weights(self):
        torch.nn.init.normal_(self.mask_token, std=.02)
        self.apply(self._init_weights)

    def forward(self, x, mask_ratio=0.0, max_span_length=1, use_masking=False, keep_mask=None):
        if keep_mask is None and use_masking:      # the span mask covers the real tokens (HTR_VT.py:221-229 on x)
            keep_mask = self.generate_span_mask(self.tokens, mask_ratio, max_span_length)
        return super().forward(x, keep_mask=keep_mask)


def create_model(nb_cls, img_size, **kwargs):
    return MaskedAutoencoderViT(nb_cls, img_size=img_size, patch_size=(4, 64), embed_dim=768, depth=4, num_heads=6,
                                mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
