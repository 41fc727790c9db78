"""Parameter containers of the LGP fork's blocks, same classes, constructor signatures, module tree and state_dict keys as
model_lgp/model/plg.py.  They only OWN parameters: the block's arithmetic runs in the HIP kernels driven by
htrvt_amd.engine.Engine (csrc/lgp.hip for the window attention, the pooling + LayerNorm and the scaled up-sampling), so
calling `.forward` on one of them is an error on purpose."""
import torch
import torch.nn as nn

import htrvt_amd                        # noqa: F401  (loads libhtrvt_hip.so or raises)
from htrvt_amd.model.HTR_VT import Mlp, _no_eager


class PooledGlobalMHSA(nn.Module):
    """adaptive average pooling to min(g_tokens, N) tokens, LayerNorm without affine, attention, linear up-sampling,
    times sigmoid(logit_alpha) (plg.py:14-76)"""

    def __init__(self, dim, num_heads, g_tokens=64, pool='avg', qkv_bias=True, attn_drop=0., proj_drop=0., alpha_init=0.4):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.g_tokens = g_tokens
        assert pool in ('avg', 'max')
        if pool != 'avg':
            raise NotImplementedError("PooledGlobalMHSA(pool='max') is not implemented: the pooling kernel averages (pool='avg')")
        self.pool = pool
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.branch_norm = nn.LayerNorm(dim, elementwise_affine=False)
        logit = torch.log(torch.tensor(alpha_init) / (1 - torch.tensor(alpha_init)))
        self.logit_alpha = nn.Parameter(logit)

    forward = _no_eager


class LayerScale(nn.Module):
    def __init__(self, dim, init_values: float = 1e-5, inplace: bool = False):
        super().__init__()
        val = 1.0 if init_values is None else float(init_values)
        self.gamma = nn.Parameter(torch.ones(dim) * val)
        self.inplace = inplace

    forward = _no_eager


class WindowMHSA1D(nn.Module):
    """self-attention in non-overlapping windows of `window_size` tokens; the sequence is zero-padded on the right in front
    of the qkv Linear, so padding slots act as keys equal to the qkv bias (plg.py:90-137)"""

    def __init__(self, dim, num_heads, window_size, qkv_bias=True, attn_drop=0., proj_drop=0.):
        super().__init__()
        assert dim % num_heads == 0
        self.win = window_size
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    forward = _no_eager


class GlobalMHSA(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias=True, attn_drop=0., proj_drop=0.):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    forward = _no_eager


class LocalGlobalParallelBlockSimple(nn.Module):
    def __init__(self, dim, num_heads, window_size=12, mlp_ratio=4.0, qkv_bias=True, drop=0.0, attn_drop=0.0, init_values=None,
                 drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, g_tokens=64, pool='avg', alpha_init=0.4):
        super().__init__()
        if drop or attn_drop or drop_path or init_values or not qkv_bias or act_layer is not nn.GELU:
            raise NotImplementedError("LocalGlobalParallelBlockSimple: dropout, drop-path, LayerScale, qkv without bias and "
                                      "activations other than GELU are not implemented (the fork's create_model uses none)")
        self.norm1 = norm_layer(dim, elementwise_affine=True)
        self.local_attn = WindowMHSA1D(dim, num_heads, window_size, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.global_attn = PooledGlobalMHSA(dim, num_heads, g_tokens=g_tokens, pool=pool, qkv_bias=qkv_bias,
                                            attn_drop=attn_drop, proj_drop=drop, alpha_init=alpha_init)
        self.fuse = nn.Linear(dim * 2, dim)
        self.ls1 = nn.Identity()
        self.dp1 = nn.Identity()
        self.norm2 = norm_layer(dim, elementwise_affine=True)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.ls2 = nn.Identity()
        self.dp2 = nn.Identity()

    forward = _no_eager
