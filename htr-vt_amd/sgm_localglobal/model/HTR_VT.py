"""MI355X-native HTR-VT encoder of the SGM local-global fork behind the fork's Python API.

Drop-in for model_sgm_localglobal/model/HTR_VT.py:
    create_model(nb_cls, img_size, **kwargs) -> nn.Module
    module(x, mask_ratio=0.0, max_span_length=1, use_masking=False, return_features=False)
        -> logits [B, N, nb_cls] (whitened, as model_v1), or (logits, feats) with feats = the final norm's output
    module.forward_features(x, mask_ratio=0.0, max_span_length=1, use_masking=False) -> feats [B, N, D] float32
Same module tree, names and construction order as the fork (HTR_VT.py:333-380): the encoder is
[LocalBlock1D(window 12), LocalBlock1D(window 12, shift 6), Block, Block] -- two blocks whose attention stays inside
windows of 12 tokens, the second on the tokens rolled by 6, then two model_v1 blocks -- so `torch.manual_seed(s);
create_model(...)` gives the fork's initial state_dict, `pos_embed` included (a frozen nn.Parameter, as in model_v1).
Logits and features come from one autograd node, as in htrvt_amd.sgm.

The fork builds every block with drop=0.0, attn_drop=0.0 and no drop-path, so train mode runs as it stands: its train.py /
valid.py / test.py work unchanged.  compute_dtype: torch.float32 (default, parity) or torch.bfloat16; "split_bf16" is not
implemented."""
from functools import partial

import torch
import torch.nn as nn

try:                                    # `from model import HTR_VT` (fork layout, htr-vt_amd/sgm_localglobal on sys.path)
    from model import resnet18
except ImportError:                     # `from htrvt_amd.sgm_localglobal.model import HTR_VT`
    from . import resnet18

import htrvt_amd                        # noqa: F401  (loads libhtrvt_hip.so or raises)
from htrvt_amd.engine import ModelShape, stem_tokens
from htrvt_amd.model import HTR_VT as _V1
from htrvt_amd.sgm.model import HTR_VT as _SGM

Mlp, LayerNorm, _no_eager, get_2d_sincos_pos_embed = _V1.Mlp, _V1.LayerNorm, _V1._no_eager, _V1.get_2d_sincos_pos_embed

WINDOW = 12                             # HTR_VT.py:360


def _no_dropout(what, **rates):
    bad = {k: v for k, v in rates.items() if v}
    if bad:
        raise NotImplementedError(f"{what}: dropout / drop-path is not implemented ({bad}); the fork builds every block "
                                  "with 0.0")


class Attention(nn.Module):
    def __init__(self, dim, num_patches, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        assert dim % num_heads == 0, 'dim should be divisible by num_heads'
        _no_dropout("Attention", attn_drop=attn_drop, proj_drop=proj_drop)
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.num_patches = num_patches
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    forward = _no_eager


class LayerScale(nn.Module):
    """defined by the fork, built by nothing (HTR_VT.py:44-51)"""

    def __init__(self, dim, init_values=1e-5, inplace=False):
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    forward = _no_eager


class Block(nn.Module):
    def __init__(self, dim, num_heads, num_patches, mlp_ratio=4., qkv_bias=False, drop=0.0, attn_drop=0., init_values=None,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        _no_dropout("Block", drop=drop, attn_drop=attn_drop, drop_path=drop_path)
        if init_values:
            raise NotImplementedError("Block: LayerScale (init_values) is not implemented; the fork builds none")
        if act_layer is not nn.GELU:
            raise NotImplementedError("Block: the MLP kernels apply GELU")
        self.norm1 = norm_layer(dim, elementwise_affine=True)
        self.attn = Attention(dim, num_patches, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = norm_layer(dim, elementwise_affine=True)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    forward = _no_eager


class WindowMHSA1D(nn.Module):
    """attention inside windows of `window_size` tokens of the sequence rolled by `shift` (HTR_VT.py:97-152); the padding
    slots of the ragged last window are rows equal to the qkv bias, nothing is masked across the wrap"""

    def __init__(self, dim, num_heads, window_size, shift=0, qkv_bias=True, attn_drop=0., proj_drop=0.):
        super().__init__()
        assert dim % num_heads == 0
        _no_dropout("WindowMHSA1D", attn_drop=attn_drop, proj_drop=proj_drop)
        self.win = window_size
        self.shift = shift
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    forward = _no_eager


class PooledGlobalMHSA(nn.Module):
    """defined by the fork, built by nothing (HTR_VT.py:156-207)"""

    def __init__(self, dim, num_heads, g_tokens=64, pool='avg', qkv_bias=True, attn_drop=0., proj_drop=0.):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.g_tokens = g_tokens
        assert pool in ('avg', 'max')
        self.pool = pool
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.norm = nn.LayerNorm(dim, elementwise_affine=False)

    forward = _no_eager


class LocalBlock1D(nn.Module):
    """Pre-LN -> WindowMHSA1D -> + residual -> Pre-LN -> MLP -> + residual (HTR_VT.py:211-227)"""

    def __init__(self, dim, num_heads, window, shift=False, mlp_ratio=4., qkv_bias=True, drop=0., attn_drop=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        _no_dropout("LocalBlock1D", drop=drop, attn_drop=attn_drop)
        if act_layer is not nn.GELU:
            raise NotImplementedError("LocalBlock1D: the MLP kernels apply GELU")
        if not qkv_bias:
            raise NotImplementedError("LocalBlock1D: qkv_bias=False (the window kernel builds its padding rows from the bias)")
        self.norm1 = norm_layer(dim, elementwise_affine=True)
        self.attn = WindowMHSA1D(dim, num_heads, window, shift=window // 2 if shift else 0, qkv_bias=qkv_bias,
                                 attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = norm_layer(dim, elementwise_affine=True)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    forward = _no_eager


class LocalGlobalParallelBlock(nn.Module):
    """defined by the fork, built by nothing (HTR_VT.py:230-255)"""

    def __init__(self, dim, num_heads, window, g_tokens=64, pool='avg', mlp_ratio=4., qkv_bias=True, drop=0., attn_drop=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim, elementwise_affine=True)
        self.local_attn = WindowMHSA1D(dim, num_heads, window, shift=0, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.global_attn = PooledGlobalMHSA(dim, num_heads, g_tokens=g_tokens, pool=pool, qkv_bias=qkv_bias,
                                            attn_drop=attn_drop, proj_drop=drop)
        self.fuse = nn.Linear(dim * 2, dim)
        self.norm2 = norm_layer(dim, elementwise_affine=True)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    forward = _no_eager


class GlobalPooledBlock(nn.Module):
    """defined by the fork, built by nothing (HTR_VT.py:258-275)"""

    def __init__(self, dim, num_heads, g_tokens=64, pool='avg', mlp_ratio=4., qkv_bias=True, drop=0., attn_drop=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim, elementwise_affine=True)
        self.attn = PooledGlobalMHSA(dim, num_heads, g_tokens=g_tokens, pool=pool, qkv_bias=qkv_bias, attn_drop=attn_drop,
                                     proj_drop=drop)
        self.norm2 = norm_layer(dim, elementwise_affine=True)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    forward = _no_eager


class MaskedAutoencoderViT(_SGM.MaskedAutoencoderViT):
    """HTR-VT encoder of the SGM local-global fork; forward / feature tap / span mask / engines as the model_sgm_2 drop-in"""

    def __init__(self, nb_cls=80, img_size=[512, 32], patch_size=[8, 32], embed_dim=1024, depth=24, num_heads=16,
                 mlp_ratio=4., norm_layer=nn.LayerNorm, compute_dtype=torch.float32):
        nn.Module.__init__(self)
        if compute_dtype == "split_bf16":
            raise NotImplementedError("the SGM local-global model has no split_bf16 path: use compute_dtype=torch.float32 "
                                      "(parity) or torch.bfloat16")
        self.layer_norm = LayerNorm()
        self.patch_embed = resnet18.ResNet18(embed_dim)
        self.grid_size = [img_size[0] // patch_size[0], img_size[1] // patch_size[1]]
        self.embed_dim = embed_dim
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.mask_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches, embed_dim), requires_grad=False)
        if img_size[0] != 64:      # the stem leaves H' = H / 64 rows of tokens; the windows are laid along one row
            raise NotImplementedError(f"the SGM local-global model is built for 64-pixel lines (img_size[0] = {img_size[0]}): "
                                      "windows over the tokens of a taller stem grid are not implemented")
        if self.num_patches != stem_tokens(img_size[0], img_size[1]):     # the fork fails at `x + self.pos_embed` here
            raise ValueError(f"img_size {tuple(img_size)} with patch_size {tuple(patch_size)}: pos_embed has "
                             f"{self.num_patches} rows, the stem leaves {stem_tokens(img_size[0], img_size[1])} tokens")
        # the fork builds these four blocks whatever `depth` says (HTR_VT.py:364-375)
        self.blocks = nn.ModuleList([
            LocalBlock1D(embed_dim, num_heads, window=WINDOW, shift=False, mlp_ratio=mlp_ratio, qkv_bias=True, drop=0.0,
                         attn_drop=0.0, act_layer=nn.GELU, norm_layer=norm_layer),
            LocalBlock1D(embed_dim, num_heads, window=WINDOW, shift=True, mlp_ratio=mlp_ratio, qkv_bias=True, drop=0.0,
                         attn_drop=0.0, act_layer=nn.GELU, norm_layer=norm_layer),
            Block(embed_dim, num_heads, self.num_patches, mlp_ratio, qkv_bias=True, norm_layer=norm_layer),
            Block(embed_dim, num_heads, self.num_patches, mlp_ratio, qkv_bias=True, norm_layer=norm_layer)])
        self.norm = norm_layer(embed_dim, elementwise_affine=True)
        self.head = nn.Linear(embed_dim, nb_cls)
        self.initialize_weights()
        eps = {m.eps for m in self.modules() if isinstance(m, nn.LayerNorm)}
        assert len(eps) == 1, f"one LayerNorm eps per model expected, got {eps}"
        self._shape = ModelShape(nb_cls, img_size, embed_dim, len(self.blocks), num_heads, mlp_ratio, patch_size,
                                 ln_eps=eps.pop(), local=self.block_kinds())
        self.compute_dtype = compute_dtype
        self._engines = {}

    def block_kinds(self):
        """per block (window, shift) of a LocalBlock1D, None of a full-attention Block: what ModelShape(local=...) takes"""
        return [(b.attn.win, b.attn.shift % b.attn.win) if isinstance(b, LocalBlock1D) else None for b in self.blocks]


def create_model(nb_cls, img_size, **kwargs):
    return MaskedAutoencoderViT(nb_cls, img_size=img_size, patch_size=(4, 64), embed_dim=768, depth=4, num_heads=6,
                                mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
