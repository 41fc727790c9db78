"""Train-time augmentation on the device (csrc/augment.hip through htrvt_amd.augment) against the numpy
restatements of tests/augment_refs.py, which tests/test_augment_cpu.py pins to the installed Pillow and scipy.

Every stage runs at (H, W) = (8, 40), (64, 136) -- no multiple of 16 or 64 -- and (64, 512), B = 3 with the middle image's
stage off: that image must come back bit-identical and its neighbours must not notice it.  Morphology and jitter are
integer / float32-exact and are held to equality.  The warp computes in float64 on both sides, which agree to about 1e-12
before the final truncation and so can part only where a value sits on an integer: the gate is |got - ref| <= 1 at every
pixel, and on noise images (where a wrong tap would show as a large difference) at most 1 % of an image's pixels may
differ at all, so that the one-level allowance cannot hide a shifted image.  An all-255 image gets the one-level gate only:
there (1 - t) * 255 + t * 255 flickers between 254 and 255 in the reference's own arithmetic."""
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_refs as A

pytestmark = pytest.mark.gpu

SHAPES = [(8, 40), (64, 136), (64, 512)]
ON = np.array([True, False, True])
FACTORS = [0.6, 0.999, 1.0, 1.0001, 1.4] + [float(f) for f in np.random.default_rng(0).uniform(0.6, 1.4, 50).astype(np.float32)]


def _args(**kw):
    d = dict(proj=8, dila_ero_max_kernel=3, dila_ero_iter=1, jitter_brightness=0.4, jitter_contrast=0.4,
             jitter_saturation=0.4, jitter_hue=0.2)
    d.update(kw)
    return SimpleNamespace(**d)


def _noise(H, W, seed, B=3):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W)).astype(np.uint8)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x))[:, None].cuda()


def _host(t):
    assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 4 and t.shape[1] == 1
    return t[:, 0].cpu().numpy()


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


# ------------------------------------------------------------------------------------------------------------ morph
@pytest.mark.parametrize("H,W", SHAPES)
def test_morph_equals_the_reference(H, W):
    from htrvt_amd import augment
    x = _noise(H, W, 1)
    d = _dev(x)
    cases = [(r, c, it) for r in (1, 2, 3) for c in (1, 2, 3) for it in (1, 2)]
    if (H, W) == (64, 136):
        cases += [(16, 11, 1), (2, 16, 1), (4, 4, 5), (6, 2, 3)]         # effective extents of 16: the cap
    for rows, cols, it in cases:
        for dilate in (False, True):
            got = _host(augment.morph(d, rows, cols, it, dilate, on=ON))
            for b in range(3):
                want = A.morph(x[b], rows, cols, it, dilate) if ON[b] else x[b]
                assert np.array_equal(got[b], want), (rows, cols, it, dilate, b, np.argwhere(got[b] != want)[:4])
    assert np.array_equal(_host(d), x)            # the input is never written


# ----------------------------------------------------------------------------------------------------------- jitter
@pytest.mark.parametrize("H,W", SHAPES)
def test_jitter_equals_the_reference(H, W):
    from htrvt_amd import augment
    noise = _noise(H, W, 2)
    flat = np.stack([np.full((H, W), 77, np.uint8), noise[1], np.full((H, W), 255, np.uint8)])    # a constant and an all-255 image
    nan = float("nan")
    for x in (noise, flat):
        d = _dev(x)
        pairs = [(f, (0.7, 1.3)[i % 2]) for i, f in enumerate(FACTORS)] + [((0.8, 1.2)[i % 2], f) for i, f in enumerate(FACTORS)]
        pairs += [(nan, 1.3), (0.8, nan), (nan, nan), (0.0, 0.5), (0.5, 0.0), (2.0, 2.0)]
        for fb, fc in pairs:
            for first in (False, True):
                # image 2 takes the factors swapped: the records are per image
                b_, c_ = np.array([fb, 0.5, fc], np.float32), np.array([fc, 0.5, fb], np.float32)
                got = _host(augment.jitter(d, b_, c_, np.array([first, first, not first]), on=ON))
                want = [A.jitter(x[0], b_[0], c_[0], first), x[1], A.jitter(x[2], b_[2], c_[2], not first)]
                for b in range(3):
                    assert np.array_equal(got[b], want[b]), (fb, fc, first, b, np.argwhere(got[b] != want[b])[:4])


# ------------------------------------------------------------------------------------------------------------- warp
def _warp_gate(got, want, noise, what):
    diff = np.abs(got.astype(int) - want.astype(int))
    print(what, "max level difference", diff.max(), "pixels that differ", int((diff > 0).sum()), "of", diff.size)
    assert diff.max() <= 1, (what, int(diff.max()))
    if noise:
        assert (diff > 0).sum() <= 0.01 * diff.size, (what, int((diff > 0).sum()), diff.size)


def _seeded_warps(H, W, proj, n):
    """n drawn warp stages of three images each, by the restated draw order"""
    out, seed = [], 100
    while len(out) < n:
        _seed(seed)
        plan = A.draw_plan(3, H, W, _args(proj=proj))
        if plan["warp"] is not None:
            out.append(plan["warp"])
        seed += 1
    return out


def _run_warp(x, recs, on=ON):
    from htrvt_amd import augment
    got = _host(augment.warp(_dev(x), np.stack([r[0] for r in recs]), [r[1] for r in recs], [r[2] for r in recs], on=on))
    want = np.stack([A.warp(x[b], *recs[b][:3]) if on[b] else x[b] for b in range(len(recs))])
    return got, want


@pytest.mark.parametrize("H,W", SHAPES)
def test_warp_seeded_plans(H, W):
    x = _noise(H, W, 3)
    white = np.full((3, H, W), 255, np.uint8)
    for i, recs in enumerate(_seeded_warps(H, W, 1 if H == 8 else 8, 3)):
        got, want = _run_warp(x, recs)
        assert np.array_equal(got[1], x[1])
        for b in (0, 2):
            assert (got[b] != x[b]).mean() > 0.5          # the stage did act
            _warp_gate(got[b], want[b], True, f"seeded plan {i} image {b} {recs[b][1]}x{recs[b][2]}")
        got, want = _run_warp(white, recs)                # hand-built case 4: an all-255 image, the one-level gate only
        for b in range(3):
            _warp_gate(got[b], want[b], False, f"all-255 under seeded plan {i} image {b}")


@pytest.mark.parametrize("H,W", SHAPES)
def test_warp_hand_built_plans(H, W):
    from htrvt_amd import augment
    x = _noise(H, W, 4)
    eye = np.eye(3)
    # 1. the identity with R x C = H x W: the output is the input
    got, want = _run_warp(x, [(eye, H, W)] * 3)
    assert np.array_equal(got, x) and np.array_equal(want, x)
    # 2. a map that reads entirely outside the source: 255 everywhere
    away = np.array([[1.0, 0.0, W + 3.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    nowhere = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])          # q = 0: not a finite point
    got, want = _run_warp(x, [(away, H, W), (away, H, W), (nowhere, H, W)])
    assert (got[0] == 255).all() and (got[2] == 255).all() and np.array_equal(got[1], x[1])
    assert (want[0] == 255).all() and (want[2] == 255).all()
    # 3. R > H and C < W
    pts = [(2.5, -1.0), (1.8, H + 0.7), (W - 3.2, H - 0.3), (W - 2.1, 0.4)]
    m, R, C = augment.warp_from_points(pts, H, W)
    assert R == H + 3 and C == W - 3
    got, want = _run_warp(x, [(m, R, C), (m, R, C), (m, R, C - 1)])
    assert np.array_equal(got[1], x[1])
    for b in (0, 2):
        _warp_gate(got[b], want[b], True, f"R > H, C < W image {b}")
    # every image on
    got, want = _run_warp(x, [(m, R, C)] * 3, on=np.ones(3, bool))
    for b in range(3):
        _warp_gate(got[b], want[b], True, f"all on, image {b}")


# ------------------------------------------------------------------------------------------------------- end to end
def _batch(B, H, W, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (1, H, W)).astype(np.float32) / np.float32(255.0), f"line {i}") for i in range(B)]


def _seed_with_every_stage(B, H, W, args):
    for seed in range(400):
        _seed(seed)
        plan = A.draw_plan(B, H, W, args)
        if all(plan[k] is not None for k in ("warp", "morph", "jitter")):
            return seed, plan
    raise AssertionError("no seed with three heads")


def test_collate_end_to_end_and_into_the_model():
    import torch.nn as nn
    import htrvt_amd
    from htrvt_amd import augment
    from htrvt_amd.model import HTR_VT
    from oracle import htrvt_oracle as O
    B, H, W = 4, 64, 512
    args = _args()
    batch = _batch(B, H, W, 6)
    u8 = np.stack([np.uint8(im[0] * 255) for im, _ in batch])
    seed, plan = _seed_with_every_stage(B, H, W, args)
    want, stages = A.collate(u8, plan)

    _seed(seed)
    out, labels = htrvt_amd.SameTrCollate(batch, args)
    assert labels == tuple(lbl for _, lbl in batch)
    assert out.shape == (B, 1, H, W)
    got = _host(out)
    for b in range(B):
        _warp_gate(got[b], want[b], True, f"whole pipeline, image {b}")

    # stage by stage: the warp within its gate, morphology and jitter exact on equal inputs
    d = _dev(u8)
    w = augment.warp(d, np.stack([r[0] for r in plan["warp"]]), [r[1] for r in plan["warp"]], [r[2] for r in plan["warp"]])
    for b in range(B):
        _warp_gate(_host(w)[b], stages["warp"][b], True, f"warp stage, image {b}")
    rows, cols, it, dil = plan["morph"]
    m = augment.morph(w, rows, cols, it, dil)
    assert np.array_equal(_host(m), np.stack([A.morph(im, rows, cols, it, dil) for im in _host(w)]))
    nan = float("nan")
    fb, fc, first = zip(*[(nan if b_ is None else b_, nan if c_ is None else c_, f) for b_, c_, f in plan["jitter"]])
    j = augment.jitter(m, fb, fc, first)
    assert np.array_equal(_host(j), np.stack([A.jitter(im, *rec) for im, rec in zip(_host(m), plan["jitter"])]))
    assert torch.equal(j, out)                           # the three stages alone = apply_plan

    # a seeded call repeated
    _seed(seed)
    again, _ = htrvt_amd.SameTrCollate(batch, args)
    assert torch.equal(again, out)

    # straight into the model: the uint8 batch is read as value / 255, no float copy
    cfg = O.Config(80, (64, 512), embed_dim=64, depth=2, num_heads=2)
    model = HTR_VT.MaskedAutoencoderViT(80, img_size=[64, 512], patch_size=(4, 64), embed_dim=64, depth=2, num_heads=2, mlp_ratio=4,
                                        norm_layer=partial(nn.LayerNorm, eps=1e-6))
    model.load_state_dict(O.init_state_dict(cfg, seed=7, randomize_affine=True), strict=True)
    model = model.cuda().eval()
    with torch.no_grad():
        y_u8 = model(out)
        y_f = model(torch.from_numpy(got[:, None].astype(np.float32) / np.float32(255.0)).cuda())
    assert torch.isfinite(y_u8).all() and torch.equal(y_u8, y_f)


def test_apply_plan_skips_the_stages_whose_coin_came_up_tails():
    from htrvt_amd import augment
    B, H, W = 3, 64, 136
    x = _noise(H, W, 7)
    d = _dev(x)
    seen = set()
    for seed in range(12):
        _seed(seed)
        want_plan = A.draw_plan(B, H, W, _args())
        _seed(seed)
        plan = augment.draw_plan(B, H, W, _args())
        key = tuple(want_plan[k] is not None for k in ("warp", "morph", "jitter"))
        seen.add(key)
        got = _host(augment.apply_plan(d, plan))
        want, _ = A.collate(x, want_plan)
        if not any(key):
            assert np.array_equal(got, x)
        elif not key[0]:
            assert np.array_equal(got, want), key         # no warp in the plan: exact
        else:
            for b in range(B):
                _warp_gate(got[b], want[b], True, f"plan {key} image {b}")
        assert np.array_equal(_host(d), x)
    assert len(seen) >= 4


def test_wrong_tensors_are_refused_before_any_launch():
    from htrvt_amd import augment
    x = _dev(_noise(8, 40, 8))
    with pytest.raises(ValueError, match="uint8"):
        augment.morph(x.float(), 2, 2)
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        augment.apply_plan(x[:, 0], augment.Plan(3, 8, 40))
    with pytest.raises(ValueError, match="as the plan was drawn"):
        augment.apply_plan(x, augment.Plan(2, 8, 40))
    with pytest.raises(ValueError, match="at most 16"):
        augment.morph(x, 17, 1)
    with pytest.raises(ValueError, match="0.19"):
        augment.warp(x, np.tile(np.eye(3), (3, 1, 1)), [12, 8, 8], [40, 40, 40])
