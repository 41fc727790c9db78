"""Inputs of the SGM local-global fixture (tests/golden/sgm_localglobal.npz), regenerated from seeds on both sides: the
tool that runs the reference (tools/make_goldens_sgm_localglobal.py) and the tests; only the reference's outputs are stored.
Seeds, perturb(), the tiny batch and the sampling of large tensors are those of the LGP fixture (tests/lgp_cases.py)."""
import numpy as np
import torch

from lgp_cases import FULL_GRAD, MASK_RATIO, MASK_SEED, MAX_SPAN, NB_CLS, d768_images, perturb, sample_index, tiny_batch  # noqa: F401

# The tiny model: d256, 4 heads, blocks [(12, 0), (12, 6), None, None].  64 x 256 -> N = 64 (pad 8; the wrap window of the
# shifted block holds tokens 58 ... 63, 0 ... 5, its ragged window tokens 54 ... 57); 64 x 800 -> N = 200 (pad 4; wrap window
# 194 ... 199, 0 ... 5, ragged window tokens 186 ... 193).  The fork's position table has grid[0] * grid[1] = (64 // ph) *
# (W // pw) rows and must have as many as the stem leaves tokens (W / 4), or the fork itself fails at `x + pos_embed`:
# create_model's patch_size (4, 64) does that for every W that is a multiple of 64, so 256 keeps it; 800 is none, and takes
# the patch size (64, 4) whose grid [1, 200] is the stem's.  Both sides build the model with the same arguments.
TINY = {256: (4, 64), 800: (64, 4)}
TINY_WIDTHS = tuple(TINY)
TINY_KW = dict(embed_dim=256, depth=4, num_heads=4, mlp_ratio=4)
KINDS = [(12, 0), (12, 6), None, None]
FEAT_SEED, FEAT_SCALE = 77, 0.02  # R of the feature term of the loss: loss_ctc + sum(feats * R)
FULL_ACT = 16384                  # logits / features up to this size are stored whole, larger ones as a fixed sample
ACT_SAMPLE = 8192


def feature_weights(B, N, D):
    """the seeded R [B, N, D] float32: d loss / d feats = R, so the feature tap's gradient runs without the SGM head"""
    r = np.random.default_rng(FEAT_SEED + N)
    return torch.from_numpy((FEAT_SCALE * r.standard_normal((B, N, D))).astype(np.float32))


def act_index(n):
    return sample_index(n, ACT_SAMPLE)
