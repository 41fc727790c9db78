"""MI355X-native HTR-VT encoder of the SGM fork model_sgm_2 behind the fork's Python API.

Drop-in for model_sgm_2/model/HTR_VT.py: model_v1's network (same module tree, state_dict and initialisation: this class
subclasses the model_v1 drop-in) plus the feature tap the SGM head trains on:
    module(x, mask_ratio=0.0, max_span_length=1, use_masking=False, return_features=False)
        -> logits [B, N, nb_cls], or (logits, feats) with feats = the final norm's output [B, N, D] float32
    module.forward_features(x, mask_ratio=0.0, max_span_length=1, use_masking=False) -> feats
Logits and features come from ONE autograd node over the engine's kernel sequence; a loss on the features is
back-propagated through the final norm into the encoder (the fork does not detach them).  The logits are bitwise those of
a call without features.  split_bf16 has no feature output (NotImplementedError).
"""
from functools import partial

import torch
import torch.nn as nn

import htrvt_amd                        # noqa: F401  (loads libhtrvt_hip.so or raises)
from htrvt_amd.model import HTR_VT as _V1

Mlp, Attention, Block, LayerNorm = _V1.Mlp, _V1.Attention, _V1.Block, _V1.LayerNorm
get_2d_sincos_pos_embed = _V1.get_2d_sincos_pos_embed


class _HTRVTFeaturesFunction(torch.autograd.Function):
    """_V1._HTRVTFunction with the final norm's output as a second result; either output may go unused"""

    @staticmethod
    def forward(ctx, module, img, keep, train, need, names, *tensors):
        ctx.set_materialize_grads(False)         # an unused output arrives as None: no zero tensor, no work for it
        eng = module._engine(img.device)
        P = dict(zip(names, tensors))
        y, feats = eng.forward(P, img, keep_mask=keep, train=train, save=need, want_features=True)
        if need:
            ctx.saved_acts, eng.saved = eng.saved, None
            ctx.eng, ctx.names, ctx.P = eng, names, P
        else:
            ctx.mark_non_differentiable(y, feats)
        return y, feats

    @staticmethod
    def backward(ctx, dy, dfeats):
        eng, names, P = ctx.eng, ctx.names, ctx.P
        G = {n: torch.zeros_like(t) for n, t in P.items() if t.requires_grad}
        if dy is not None or dfeats is not None:
            eng.saved = ctx.saved_acts
            eng.backward(P, G, None if dy is None else dy.contiguous().float(),
                         dfeats=None if dfeats is None else dfeats.contiguous().float())
        ctx.saved_acts = None
        return (None, None, None, None, None, None) + tuple(G.get(n) for n in names)


class MaskedAutoencoderViT(_V1.MaskedAutoencoderViT):
    """HTR-VT encoder of model_sgm_2: model_v1 plus forward_features / return_features"""

    def forward_features(self, x, mask_ratio=0.0, max_span_length=1, use_masking=False, keep_mask=None):
        return self.forward(x, mask_ratio, max_span_length, use_masking, return_features=True, keep_mask=keep_mask)[1]

    def forward(self, x, mask_ratio=0.0, max_span_length=1, use_masking=False, return_features=False, keep_mask=None):
        if not return_features:
            return super().forward(x, mask_ratio, max_span_length, use_masking, keep_mask=keep_mask)
        if self.compute_dtype == "split_bf16":
            raise NotImplementedError("split_bf16 has no feature output (return_features=True): use "
                                      "compute_dtype=torch.float32 (parity) or torch.bfloat16")
        if not x.is_cuda:
            raise RuntimeError("htrvt_amd runs on an MI355X only: move the model and the input to cuda "
                               "(no CPU / eager fallback exists)")
        if keep_mask is None and use_masking:
            keep_mask = self.generate_span_mask(self.num_patches, mask_ratio, max_span_length)
        names, tensors = [], []
        for n, t in self.state_dict(keep_vars=True).items():
            names.append(n)
            tensors.append(t)
        x = x.contiguous() if x.dtype == torch.uint8 else x.contiguous().float()
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("htrvt_amd computes no gradient with respect to the input image (d loss / d image): "
                               "detach the image, or call under torch.no_grad()")
        need = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
        return _HTRVTFeaturesFunction.apply(self, x, keep_mask, self.training, need, tuple(names), *tensors)


def create_model(nb_cls, img_size, **kwargs):
    return MaskedAutoencoderViT(nb_cls, img_size=img_size, patch_size=(4, 64), embed_dim=768, depth=4, num_heads=6,
                                mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
