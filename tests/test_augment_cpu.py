"""Train-time augmentation, host side: tests/augment_refs.py against the installed Pillow and scipy (the
libraries the reference's collate function stands on -- skimage, cv2 and torchvision -- are restated from behaviour),
draw_plan against a straight-line restatement of the reference's draw order, and every refusal, none of which needs or
touches a GPU."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_refs as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = [0.6, 0.999, 1.0, 1.0001, 1.4]


def _args(**kw):
    d = dict(proj=8, dila_ero_max_kernel=3, dila_ero_iter=1, jitter_brightness=0.4, jitter_contrast=0.4,
             jitter_saturation=0.4, jitter_hue=0.2)
    d.update(kw)
    return SimpleNamespace(**d)


def _factors():
    return FACTORS + [float(f) for f in np.random.default_rng(0).uniform(0.6, 1.4, 50).astype(np.float32)]


def _level_images():
    rng = np.random.default_rng(1)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    noise = rng.permutation(np.arange(512) % 256).astype(np.uint8).reshape(16, 32)     # all 256 levels, twice
    dark = (noise // 3).astype(np.uint8)
    return [ramp, noise, dark, np.full((8, 8), 77, np.uint8), np.full((8, 8), 255, np.uint8)]


def test_blend_reference_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    for img in _level_images():
        pil = Image.fromarray(img)
        for f in _factors():
            b = np.array(ImageEnhance.Brightness(pil).enhance(f))
            c = np.array(ImageEnhance.Contrast(pil).enhance(f))
            assert np.array_equal(A.brightness(img, f), b), f
            assert np.array_equal(A.contrast(img, f), c), f
            for g in (0.7, 1.3):      # both orders
                bc = np.array(ImageEnhance.Contrast(ImageEnhance.Brightness(pil).enhance(f)).enhance(g))
                cb = np.array(ImageEnhance.Brightness(ImageEnhance.Contrast(pil).enhance(g)).enhance(f))
                assert np.array_equal(A.jitter(img, f, g, False), bc), (f, g)
                assert np.array_equal(A.jitter(img, f, g, True), cb), (f, g)
    x = _level_images()[1]
    assert np.array_equal(A.jitter(x, float("nan"), None, True), x)


def test_morph_reference_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (13, 21)).astype(np.uint8)

    def erode(x, rows, cols):
        # cv2's anchor (rows // 2, cols // 2) is scipy's centre for a footprint of that shape with origin 0
        return ndi.grey_erosion(x, footprint=np.ones((rows, cols)), mode="constant", cval=255)

    for rows in (1, 2, 3):
        for cols in (1, 2, 3):
            e1, d1 = erode(img, rows, cols), 255 - erode(255 - img, rows, cols)
            assert np.array_equal(A.morph(img, rows, cols, 1, False), e1), (rows, cols)
            assert np.array_equal(A.morph(img, rows, cols, 1, True), d1), (rows, cols)
            assert np.array_equal(A.morph(img, rows, cols, 2, False), erode(e1, rows, cols)), (rows, cols)
            assert np.array_equal(A.morph(img, rows, cols, 2, True), 255 - erode(255 - d1, rows, cols)), (rows, cols)


def test_warp_reference_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    H, W = 16, 40
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    np.random.seed(5)
    from htrvt_amd import augment
    for _ in range(4):
        m, R, C = augment.warp_from_points(augment._draw_warp_points(H, W, 2.0), H, W)
        r, c = np.mgrid[0:R, 0:C].astype(np.float64)
        p = np.einsum("ij,jrc->irc", m, np.stack([c, r, np.ones_like(r)]))
        want = ndi.map_coordinates(img.astype(np.float64), [p[1] / p[2], p[0] / p[2]], order=1, mode="grid-constant", cval=255)
        got = A.warp_stage(img, m, R, C)
        assert got.shape == (R, C) and np.abs(got - want).max() < 1e-9
        for shape in ((H, W), (H + 3, W - 5), (H - 2, W + 7)):
            z = ndi.zoom(got, (shape[0] / R, shape[1] / C), order=1, mode="reflect", grid_mode=True)
            assert z.shape == shape and np.abs(A.resize_stage(got, *shape) - z).max() < 1e-9


def test_homography_maps_the_source_points_onto_the_corners():
    from htrvt_amd import augment
    np.random.seed(11)
    for H, W, proj in [(64, 512, 8), (8, 40, 1), (64, 136, 8), (32, 100, 0)]:
        for _ in range(5):
            pts = np.array(augment._draw_warp_points(H, W, proj))
            m, R, C = augment.warp_from_points(pts, H, W)
            assert m[2, 2] == 1.0
            assert R == int(np.around(np.ptp(pts[:, 1]) + 1)) and C == int(np.around(np.ptp(pts[:, 0]) + 1))
            corners = np.array([(0, 0), (0, H - 1), (W - 1, H - 1), (W - 1, 0)], np.float64)
            for (x, y), want in zip(pts - pts.min(0), corners):
                u, v, q = m @ np.array([x, y, 1.0])
                assert abs(u / q - want[0]) < 1e-9 and abs(v / q - want[1]) < 1e-9
            assert np.abs(m - A.solve_homography(pts - pts.min(0), corners)).max() < 1e-9


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


def _state():
    st = np.random.get_state()
    return st[1].tobytes(), st[2], torch.get_rng_state().numpy().tobytes()


@pytest.mark.parametrize("args", [_args(), _args(jitter_contrast=0.0), _args(jitter_brightness=0, jitter_hue=0), _args(proj=0),
                                  _args(dila_ero_iter=2, dila_ero_max_kernel=2)])
def test_draw_plan_follows_the_reference_draw_order(args):
    from htrvt_amd import augment
    B, H, W = 3, 64, 136
    seen = set()
    for seed in range(24):
        _seed(seed)
        want = A.draw_plan(B, H, W, args)
        want_state = _state()
        _seed(seed)
        plan = augment.draw_plan(B, H, W, args)
        assert _state() == want_state, seed
        assert (plan.B, plan.H, plan.W) == (B, H, W)
        seen.add((plan.warp is not None, plan.morph is not None, plan.jitter is not None))
        assert (plan.warp is None) == (want["warp"] is None)
        if plan.warp is not None:
            for b, (m, R, C, _) in enumerate(want["warp"]):
                assert np.array_equal(plan.warp.m[b], m) and plan.warp.rows[b] == R and plan.warp.cols[b] == C
            assert plan.warp.on.all()
            if args.proj == 0:
                assert (plan.warp.rows == H + 1).all() and (plan.warp.cols == W + 1).all()
        assert (plan.morph is None) == (want["morph"] is None)
        if plan.morph is not None:
            assert (plan.morph.rows, plan.morph.cols, plan.morph.iterations, plan.morph.dilate) == want["morph"]
        assert (plan.jitter is None) == (want["jitter"] is None)
        if plan.jitter is not None:
            for b, (fb, fc, first) in enumerate(want["jitter"]):
                for got, f in ((plan.jitter.brightness[b], fb), (plan.jitter.contrast[b], fc)):
                    assert np.isnan(got) if f is None else got == np.float32(f)
                assert plan.jitter.contrast_first[b] == first
            assert np.isnan(plan.jitter.brightness).all() == (args.jitter_brightness == 0)
            assert np.isnan(plan.jitter.contrast).all() == (args.jitter_contrast == 0)
    assert len({s[0] for s in seen}) == 2 and len({s[1] for s in seen}) == 2 and len({s[2] for s in seen}) == 2


def test_the_element_keeps_the_reference_row_column_swap():
    """np.ones((kernel_w, kernel_h)): the SECOND torch.randint is the row count"""
    from htrvt_amd import augment
    checked = 0
    for seed in range(40):
        _seed(seed)
        plan = augment.draw_plan(2, 64, 136, _args(dila_ero_max_kernel=3))
        if plan.morph is None or plan.morph.rows == plan.morph.cols:
            continue
        torch.manual_seed(seed)       # the morphology's draws are the first that torch's generator serves
        kernel_h, kernel_w = int(torch.randint(1, 4, (1,))), int(torch.randint(1, 4, (1,)))
        assert (plan.morph.rows, plan.morph.cols) == (kernel_w, kernel_h)
        checked += 1
    assert checked > 0


def test_refusals_are_decided_on_the_host():
    from htrvt_amd import augment
    B = 2
    on = np.ones(B, bool)
    eye = np.tile(np.eye(3), (B, 1, 1))
    # sigma: H = 32 under --proj 8 can need a 49-row warped image
    bad = augment.Plan(B, 32, 100, warp=augment.WarpPlan(eye, np.array([45, 32]), np.array([100, 100]), on))
    with pytest.raises(ValueError, match="0.19"):
        augment.validate_plan(bad)
    with pytest.raises(ValueError, match="0.19"):
        augment.apply_plan(torch.zeros(B, 1, 32, 100, dtype=torch.uint8), bad)
    hit = 0
    for seed in range(40):
        np.random.seed(seed)
        try:
            augment.draw_plan(4, 32, 100, _args())
        except ValueError as e:
            assert "0.19" in str(e)
            hit += 1
    assert hit > 0
    augment.validate_plan(augment.Plan(B, 64, 100, warp=augment.WarpPlan(eye, np.array([88, 64]), np.array([100, 138]), on)))
    off = augment.Plan(B, 32, 100, warp=augment.WarpPlan(eye, np.array([45, 32]), np.array([100, 100]), np.array([False, True])))
    augment.validate_plan(off)        # an image that is off is not warped: its record is not judged
    # extent
    for rows, cols, it in [(17, 1, 1), (1, 17, 1), (6, 2, 4), (2, 3, 8)]:
        with pytest.raises(ValueError, match="at most 16"):
            augment.validate_plan(augment.Plan(B, 64, 100, morph=augment.MorphPlan(rows, cols, it, False, on)))
    augment.validate_plan(augment.Plan(B, 64, 100, morph=augment.MorphPlan(16, 6, 1, True, on)))
    augment.validate_plan(augment.Plan(B, 64, 100, morph=augment.MorphPlan(4, 2, 5, True, on)))
    with pytest.raises(ValueError, match="1024"):
        augment.validate_plan(augment.Plan(B, 1025, 100))
    # tensors
    ok = augment.Plan(B, 64, 100, morph=augment.MorphPlan(2, 2, 1, False, on))
    with pytest.raises(ValueError, match="device"):
        augment.apply_plan(torch.zeros(B, 1, 64, 100, dtype=torch.uint8), ok)
    with pytest.raises(ValueError, match="device"):
        augment.morph(torch.zeros(B, 1, 64, 100, dtype=torch.uint8), 2, 2)
    with pytest.raises(ValueError, match="device"):
        augment.apply_plan(np.zeros((B, 1, 64, 100), np.uint8), ok)


def test_collate_refuses_to_run_in_a_loader_worker(monkeypatch):
    import htrvt_amd
    assert htrvt_amd.SameTrCollate is htrvt_amd.augment.SameTrCollate
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: SimpleNamespace(id=0))
    batch = [(np.ones((1, 8, 40), np.float32), "a")]
    before = _state()
    with pytest.raises(RuntimeError, match="worker"):
        htrvt_amd.SameTrCollate(batch, _args())
    assert _state() == before         # refused before the first draw


def test_c_entry_points_refuse_before_any_launch():
    """null pointers, bad geometry and the caps through the C ABI: decided on the host (no GPU here, nothing could launch)"""
    from htrvt_amd._lib import lib
    p = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused
    q = ctypes.c_void_p(8192)
    assert lib.htrvt_aug_warp(None, p, q, 1, 8, 8, None) == -1 and b"null" in lib.htrvt_last_error()
    assert lib.htrvt_aug_jitter(p, None, q, 1, 8, 8, None) == -1 and b"null" in lib.htrvt_last_error()
    assert lib.htrvt_aug_morph(p, p, None, 1, 8, 8, 1, 1, 1, 0, None) == -1 and b"null" in lib.htrvt_last_error()
    assert lib.htrvt_aug_warp(p, p, p, 1, 8, 8, None) == -1 and b"same buffer" in lib.htrvt_last_error()
    for B, H, W in [(0, 8, 8), (1, 0, 8), (1, 8, 0), (65536, 8, 8), (1, 1025, 8), (1, 8, 16385)]:
        assert lib.htrvt_aug_warp(p, p, q, B, H, W, None) == -1 and b"bad shape" in lib.htrvt_last_error()
        assert lib.htrvt_aug_jitter(p, p, q, B, H, W, None) == -1
        assert lib.htrvt_aug_morph(p, p, q, B, H, W, 1, 1, 1, 0, None) == -1
    for rows, cols, it in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (17, 1, 1), (6, 2, 4), (2, 1 << 30, 1 << 30)]:
        assert lib.htrvt_aug_morph(p, p, q, 1, 8, 8, rows, cols, it, 0, None) == -1
    assert lib.htrvt_aug_morph(p, p, q, 1, 8, 8, 6, 2, 4, 0, None) == -1 and b"exceeds 16" in lib.htrvt_last_error()


def test_table_records_match_the_header(tmp_path):
    from htrvt_amd import augment
    structs = {"HtrvtAugWarp": augment._WARP_DT, "HtrvtAugJitter": augment._JITTER_DT}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "htrvt.h"', "int main(void) {"]
    for cname, dt in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname in dt.names:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("caps %d %d %d %d\\n", HTRVT_AUG_MAX_B, HTRVT_AUG_MAX_H, HTRVT_AUG_MAX_W, HTRVT_AUG_MAX_EXTENT);',
              '  printf("flags %d %d %d %d\\n", HTRVT_AUG_ON, HTRVT_AUG_BRIGHTNESS, HTRVT_AUG_CONTRAST, HTRVT_AUG_CONTRAST_FIRST);',
              "  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, dt in structs.items():
        assert int(got[cname]) == dt.itemsize
        for fname in dt.names:
            assert int(got[f"{cname}.{fname}"]) == dt.fields[fname][1], (cname, fname)
    assert augment._WARP_DT["m"].shape == (9,) and augment._WARP_DT["m"].base == np.float64
    assert all(augment._WARP_DT[f] == np.int32 for f in ("rows", "cols", "on"))
    assert augment._JITTER_DT["brightness"] == np.float32 and augment._JITTER_DT["contrast"] == np.float32
    assert augment._JITTER_DT["flags"] == np.int32
    assert got["caps"].split() == [str(v) for v in (augment.MAX_B, augment.MAX_H, augment.MAX_W, augment.MAX_EXTENT)]
    assert got["flags"].split() == [str(v) for v in (augment.ON, augment.BRIGHTNESS, augment.CONTRAST, augment.CONTRAST_FIRST)]
    hdr = open(os.path.join(ROOT, "include", "htrvt.h")).read()
    for sym in ("htrvt_aug_warp", "htrvt_aug_morph", "htrvt_aug_jitter"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
