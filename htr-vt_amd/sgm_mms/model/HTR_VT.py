"""MI355X-native HTR-VT encoder of the multi-mask SGM forks behind the forks' Python API.

Drop-in for model_sgm_mms_attach/model/HTR_VT.py and model_sgm_mms_detach/model/HTR_VT.py (the same file; the two forks'
train.py differ in `feats.detach()` in front of the SGM head only).  The network is model_sgm_2's -- this class
subclasses the htrvt_amd.sgm drop-in: same module tree, state_dict and initialisation -- with ONE difference in the
forward: the forks do not whiten the input image (model_sgm_2's parameter-free LayerNorm in front of the stem is gone from
their forward_features), so this model's engine runs with ModelShape(whiten_input=False).  What the forks add is how
tokens are masked in training: per-sample random, block-wise and span masks, alone or as their union ("mms"):
    module(x, use_masking=False, return_features=False, mask_mode="mms", mask_ratio=None, max_span_length=None)
        -> logits [B, N, nb_cls], or (logits, feats) with feats = the final norm's output [B, N, D] float32
    module.forward_features(x, use_masking=False, mask_mode="mms", mask_ratio=0.5, max_span_length=8, ratios=None,
                            block_params=None) -> feats
    mask_mode: "random" | "block" | "span_old" | anything else = "mms", as HTR_VT.py:368-377 reads it
    module._mask_random_1d / _mask_block_1d / _mask_span_1d / _mask_span_old_1d / generate_mms_mask(x, ...) /
    generate_span_mask(x, mask_ratio, max_span_length): the forks' helpers, served by htrvt_amd.masking (block and span
    bookkeeping in host memory, one upload per mask, the forks' random streams draw for draw)
    module.mms_ratios: when set, the ratios of the "mms" union (the forks read it with getattr)
The mask [B, N] goes to the engine as it is: the token kernel (htrvt_pool_tokens_ps) reads one mask row per sample, its
backward and the mask token's gradient likewise.  Every call is one autograd node over the whole model, so the three
masked passes of the forks' tri_masked_loss are three stem passes and three BatchNorm buffer updates, as in the forks.

Beyond the forks' interface: `keep_mask=` (a ready [N], [B, N] or [B, N, 1] keep mask: no generator runs), `mask_device`
(where the generators draw; None = the input's device, as in the forks; "cpu" draws from the CPU generators, which is
what a CPU run of the fork consumes) and `last_keep_mask` (the float keep mask [B, N] of the last masked call, or None).
"""
from functools import partial

import torch
import torch.nn as nn

import htrvt_amd                        # noqa: F401  (loads libhtrvt_hip.so or raises)
from htrvt_amd import masking
from htrvt_amd.engine import ModelShape
from htrvt_amd.model import HTR_VT as _V1
from htrvt_amd.sgm.model import HTR_VT as _SGM

Mlp, Attention, Block, LayerNorm = _V1.Mlp, _V1.Attention, _V1.Block, _V1.LayerNorm
get_2d_sincos_pos_embed = _V1.get_2d_sincos_pos_embed


class MaskedAutoencoderViT(_SGM.MaskedAutoencoderViT):
    """HTR-VT encoder of model_sgm_mms_attach / model_sgm_mms_detach: model_sgm_2 plus the multi-mask modes"""

    mask_device = None          # None: the generators draw on the input's device (the forks' behaviour)
    last_keep_mask = None

    def __init__(self, nb_cls=80, img_size=[512, 32], patch_size=[8, 32], embed_dim=1024, depth=24, num_heads=16,
                 mlp_ratio=4., norm_layer=nn.LayerNorm, compute_dtype=torch.float32):
        super().__init__(nb_cls, img_size, patch_size, embed_dim, depth, num_heads, mlp_ratio, norm_layer, compute_dtype)
        # HTR_VT.py:360-366 of the forks: forward_features hands the image to the ResNet as it is -- model_sgm_2's
        # `x = self.layer_norm(x)` in front of the stem is gone (the parameter-free LayerNorm still follows the head)
        self._shape = ModelShape(nb_cls, img_size, embed_dim, depth, num_heads, mlp_ratio, patch_size,
                                 ln_eps=self._shape.ln_eps, whiten_input=False)

    # ---- the forks' mask helpers (HTR_VT.py:222-346) ----
    def _mask_random_1d(self, B, L, ratio, device):
        return masking.mask_random_1d(B, L, ratio, device)

    def _mask_block_1d(self, B, L, ratio, device, min_block=2):
        return masking.mask_block_1d(B, L, ratio, device, min_block)

    def _mask_span_1d(self, B, L, ratio, max_span, device):
        return masking.mask_span_1d(B, L, ratio, max_span, device)

    def _mask_span_old_1d(self, B, L, ratio, max_span, device):
        return masking.mask_span_old_1d(B, L, ratio, max_span, device)

    def generate_mms_mask(self, x, ratios=None, max_span_length=8, block_params=None):
        """x: a token tensor [B, L, D] (its shape and device are used) -> float keep mask [B, L, 1]"""
        B, L, _ = x.shape
        return self._mms(B, L, x.device, ratios, max_span_length, block_params)

    def _mms(self, B, L, device, ratios, max_span_length, block_params):
        if ratios is None:
            ratios = getattr(self, "mms_ratios", masking.DEFAULT_RATIOS)
        return masking.generate_mms_mask(B, L, device, ratios, max_span_length, block_params)

    def _keep_for(self, B, device, mask_mode, mask_ratio, max_span_length, ratios, block_params):
        """the keep mask [B, N, 1] of HTR_VT.py:368-376 for a batch of B images"""
        L = self.num_patches
        if self.mask_device is not None:
            device = self.mask_device
        if mask_mode == "random":
            return masking.keep_from_mask(self._mask_random_1d(B, L, mask_ratio, device))
        if mask_mode == "block":
            return masking.keep_from_mask(self._mask_block_1d(B, L, mask_ratio, device))
        if mask_mode == "span_old":
            return masking.keep_from_mask(self._mask_span_old_1d(B, L, mask_ratio, max_span_length, device))
        return self._mms(B, L, device, ratios, max_span_length, block_params)

    def _masked_call(self, x, use_masking, return_features, mask_mode, mask_ratio, max_span_length, ratios, block_params,
                     keep_mask):
        if not x.is_cuda:
            raise RuntimeError("htrvt_amd runs on an MI355X only: move the model and the input to cuda "
                               "(no CPU / eager fallback exists)")
        if keep_mask is None and use_masking:
            keep_mask = self._keep_for(x.shape[0], x.device, mask_mode, mask_ratio, max_span_length, ratios, block_params)
        self.last_keep_mask = None if keep_mask is None else keep_mask.detach().float().reshape(-1, self.num_patches)
        return _SGM.MaskedAutoencoderViT.forward(self, x, return_features=return_features, keep_mask=keep_mask)

    def forward_features(self, x, use_masking=False, mask_mode="mms", mask_ratio=0.5, max_span_length=8, ratios=None,
                         block_params=None, keep_mask=None):
        return self._masked_call(x, use_masking, True, mask_mode, mask_ratio, max_span_length, ratios, block_params,
                                 keep_mask)[1]

    def forward(self, x, use_masking=False, return_features=False, mask_mode="mms", mask_ratio=None, max_span_length=None,
                keep_mask=None):
        return self._masked_call(x, use_masking, return_features, mask_mode, mask_ratio, max_span_length, None, None,
                                 keep_mask)


def create_model(nb_cls, img_size, **kwargs):
    return MaskedAutoencoderViT(nb_cls, img_size=img_size, patch_size=(4, 64), embed_dim=768, depth=4, num_heads=6,
                                mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
