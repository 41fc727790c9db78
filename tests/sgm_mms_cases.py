"""Cases shared by tools/make_goldens_sgm_mms.py (which runs the reference fork model_sgm_mms_attach on the CPU) and the
tests of the drop-in htrvt_amd.sgm_mms / htrvt_amd.masking.  Both sides rebuild inputs and weights from seeds, so
tests/golden/sgm_mms.npz holds results only.

GEN_CASES: (name, generator, B, L, keyword arguments) of the mask generators, each run after random.seed(s);
torch.manual_seed(s) with s = gen_seed(index).  The fixture stores the mask, the next random.random() and torch.rand(1)
behind the call (the streams were consumed identically) and the number of loop trials the fork needed; every case ends
before the fork's cap of 10 000 trials per sample (checked when the fixture is generated).
"""
import numpy as np
import torch

SHAPES = [(1, 1), (3, 7), (4, 64), (2, 200)]
# 0; a ratio whose target rounds to 0 at every L of SHAPES but 200 (where it is 1); the span generator's three spacing
# regimes: 0.25 and exactly 0.4 (k = the span's length), 0.6 (k = 1), 0.8 (k = 0)
RATIOS = [0.0, 0.004, 0.25, 0.4, 0.6, 0.8]
MAX_SPANS = [1, 8, 300]                  # 300 > every L


def _gen_cases():
    cases = []
    for B, L in SHAPES:
        for r in RATIOS:
            cases.append((f"random.{B}x{L}.r{r}", "random", B, L, dict(ratio=r)))
            cases.append((f"block.{B}x{L}.r{r}", "block", B, L, dict(ratio=r)))
            for ms in MAX_SPANS:
                if r == 0.6 and ms == 1 and L > 1:
                    continue            # single tokens one apart cover at most half of a line: the fork runs into its cap
                cases.append((f"span.{B}x{L}.r{r}.s{ms}", "span", B, L, dict(ratio=r, max_span=ms)))
        # min_block 3 / 5: the remaining target falls below min_block after the first block or two
        cases.append((f"block.{B}x{L}.r0.3.mb3", "block", B, L, dict(ratio=0.3, min_block=3)))
        cases.append((f"block.{B}x{L}.r0.1.mb5", "block", B, L, dict(ratio=0.1, min_block=5)))
    # span_old: int(L ratio) // max_span spans -- none, one, several; max_span > L; L = 1
    for B, L, r, ms in [(4, 64, 0.1, 8), (3, 7, 0.5, 3), (4, 64, 0.3, 8), (2, 200, 0.3, 8), (2, 200, 0.6, 1), (3, 7, 0.9, 300),
                        (1, 1, 1.0, 1), (4, 64, 0.0, 8), (2, 200, 1.0, 300)]:
        cases.append((f"span_old.{B}x{L}.r{r}.s{ms}", "span_old", B, L, dict(ratio=r, max_span=ms)))
    for B, L in SHAPES:
        cases.append((f"mms.{B}x{L}.default", "mms", B, L, dict(max_span_length=8)))
        cases.append((f"mms.{B}x{L}.ratios", "mms", B, L,
                      dict(max_span_length=4, mms_ratios={"random": 0.2, "block": 0.3, "span": 0.1})))
        cases.append((f"mms.{B}x{L}.args", "mms", B, L,
                      dict(max_span_length=8, ratios={"random": 0.1, "block": 0.4}, block_params={"min_block": 3})))
    return cases


GEN_CASES = _gen_cases()


def gen_seed(index):
    return 1000 + index


# ---- the model cases: the tiny model of tests/test_sgm_gpu.py's train step (64 x 512, D = 64, 2 layers, 2 heads) on the first
# MODEL_B images of tests/golden/tiny_model.npz
MODEL_B = 2
MAX_SPAN = 8
MODES = {"random": 0.60, "block": 0.40, "span_old": 0.40, "mms": None}      # the ratios of the fork's train.py:243-247
TRI_MODES = ("random", "block", "span_old")                                  # tri_masked_loss, train.py:76-97
FEAT_WEIGHT = 1.0            # loss = ctc + FEAT_WEIGHT * mean(feats^2): both outputs of the autograd node carry a gradient
SGD_LR = 0.05
FULL_GRAD = 1024             # the scheme of tests/window_cases.py: gradients up to this size whole, larger ones as a fixed
GRAD_SAMPLE = 512            # sample of this many entries + the norm (smaller constants: the fixture stays below 1 MiB)
LOGIT_TOKENS = slice(0, None, 2)    # the train-mode logits are stored at every second token (masked and kept ones),
FEAT_TOKENS = slice(0, None, 4)     # the features at every fourth


def mode_seed(mode):
    return 500 + list(MODES).index(mode)


TRI_SEED = 77


def sample_index(n, k=GRAD_SAMPLE):
    return np.random.default_rng(n).choice(n, size=k, replace=False)


def model_config():
    from oracle import htrvt_oracle as O
    return O.Config(80, (64, 512), embed_dim=64, depth=2, num_heads=2)


def model_state_dict():
    from oracle import htrvt_oracle as O
    return O.init_state_dict(model_config(), seed=7, randomize_affine=True)


def model_batch(golden_dir):
    """(x [MODEL_B, 1, 64, 512] float32, targets int32, lengths int32) of the first MODEL_B lines of tiny_model.npz"""
    import os
    t = np.load(os.path.join(golden_dir, "tiny_model.npz"))
    lengths = t["lengths"][:MODEL_B]
    return (torch.from_numpy(t["x"][:MODEL_B]), torch.from_numpy(t["targets"][:int(lengths.sum())]),
            torch.from_numpy(lengths))


def mode_kwargs(mode):
    """the keyword arguments of the fork's compute_losses call (train.py:46-53)"""
    return dict(use_masking=True, return_features=True, mask_mode=mode, mask_ratio=MODES[mode], max_span_length=MAX_SPAN)
