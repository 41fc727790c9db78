"""Train-time augmentation on the device: the reference's collate function (data/dataset.py:13-45,
SameTrCollate -- per batch three coins; a projective warp + resize, an erosion / dilation, a colour jitter) as a host
plan and three HIP launches (csrc/augment.hip).

    draw_plan(B, H, W, args)   every random draw of one batch, from the global numpy / torch generators in the
                               reference's order.  A plain host object: needs no GPU, may run in a DataLoader worker.
    apply_plan(images, plan)   device uint8 [B,1,H,W] -> device uint8 [B,1,H,W], one launch per stage whose coin came up
                               heads, ping-pong between two buffers.
    SameTrCollate(batch, args) the reference's signature; returns the uint8 device batch the model reads as value / 255.

uint8 in, uint8 out, no float image anywhere.  Two stated deviations from the reference: the homography is
solved from the four point pairs directly (skimage: a normalised SVD; equal to rounding), and the anti-aliasing Gaussian
of a shrinking resize is left out -- a plan whose sigma exceeds MAX_SIGMA is refused."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.utils.data

from ._lib import check, lib
from .ops import ptr, stream

MAX_B, MAX_H, MAX_W = 65535, 1024, 16384     # include/htrvt.h: HTRVT_AUG_MAX_*
MAX_EXTENT = 16                              # effective rows / cols of the morphology's rectangle
MAX_SIGMA = 0.19                             # neighbour weight of the left-out Gaussian exp(-1 / (2 sigma^2)) < 1e-6
ON, BRIGHTNESS, CONTRAST, CONTRAST_FIRST = 1, 2, 4, 8


# the device tables' records, include/htrvt.h: HtrvtAugWarp, HtrvtAugJitter
_WARP_DT = np.dtype([("m", "<f8", (9,)), ("rows", "<i4"), ("cols", "<i4"), ("on", "<i4"), ("reserved_", "<i4")])
_JITTER_DT = np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("flags", "<i4"), ("reserved_", "<i4")])


@dataclass
class WarpPlan:
    """per image: m [B,3,3] float64 takes pixel (c, r) of the warped rows[b] x cols[b] image to source coordinates"""
    m: np.ndarray
    rows: np.ndarray
    cols: np.ndarray
    on: np.ndarray


@dataclass
class MorphPlan:
    """one rectangle for the batch: np.ones((rows, cols)), cv2 conventions; on [B]"""
    rows: int
    cols: int
    iterations: int
    dilate: bool
    on: np.ndarray


@dataclass
class JitterPlan:
    """per image: the two factors (float32; NaN where the strength is 0 and the step does not act), whether contrast comes
    before brightness in the drawn permutation, on [B]"""
    brightness: np.ndarray
    contrast: np.ndarray
    contrast_first: np.ndarray
    on: np.ndarray


@dataclass
class Plan:
    B: int
    H: int
    W: int
    warp: Optional[WarpPlan] = None
    morph: Optional[MorphPlan] = None
    jitter: Optional[JitterPlan] = None


def homography(src, dst):
    """the 3 x 3 map (m[2,2] = 1) with m (src_i, 1) ~ (dst_i, 1) for four point pairs [(x, y)], float64"""
    a, b = np.zeros((8, 8)), np.zeros(8)
    for i, ((x, y), (u, v)) in enumerate(zip(np.asarray(src, np.float64), np.asarray(dst, np.float64))):
        a[2 * i] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        a[2 * i + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
        b[2 * i], b[2 * i + 1] = u, v
    return np.append(np.linalg.solve(a, b), 1.0).reshape(3, 3)


def warp_from_points(pts, H, W):
    """RandomTransform (transform.py:183-219) from its four source points [(col, row)] (top-left, bottom-left,
    bottom-right, top-right): the map that sends them to the image corners, the shape of the warped image that holds
    them all, the translation into it, the normalisation.  Returns m, R, C."""
    pts = np.asarray(pts, np.float64)
    m = homography(pts, [(0, 0), (0, H - 1), (W - 1, H - 1), (W - 1, 0)])
    minc, minr = pts[:, 0].min(), pts[:, 1].min()
    maxc, maxr = pts[:, 0].max(), pts[:, 1].max()
    R, C_ = np.around((maxr - minr + 1, maxc - minc + 1))
    m = m @ np.array([[1.0, 0.0, minc], [0.0, 1.0, minr], [0.0, 0.0, 1.0]])
    return m / m[2, 2], int(R), int(C_)


def _draw_warp_points(H, W, val):
    """transform.py:164-188: the draws of one image, in its order"""
    dw, dh = (val, 0) if np.random.randint(0, 2) == 0 else (0, val)

    def rd(d):
        return np.random.uniform(-d, d)

    def fd(d):
        return np.random.uniform(-dw, d)

    tl_top = rd(dh)
    tl_left = fd(dw)
    bl_bottom = rd(dh)
    bl_left = fd(dw)
    tr_top = rd(dh)
    tr_right = fd(min(W * 3 / 4 - tl_left, dw))
    br_bottom = rd(dh)
    br_right = fd(min(W * 3 / 4 - bl_left, dw))
    return [(tl_left, tl_top), (bl_left, H - bl_bottom), (W - br_right, H - br_bottom), (W - tr_right, tr_top)]


def _randint(low, high):            # utils/utils.py:17
    return int(torch.randint(low, high, (1,)))


def _uniform(strength, lo, hi):     # torchvision ColorJitter.get_params: no draw for a step that is switched off
    return float(torch.empty(1).uniform_(lo, hi)) if strength else float("nan")


def draw_plan(B, H, W, args) -> Plan:
    """The draws of SameTrCollate for a batch of B images of H x W, consuming np.random and torch's global generator
    exactly as the reference does.  args: proj, dila_ero_max_kernel, dila_ero_iter, jitter_brightness, jitter_contrast,
    jitter_saturation, jitter_hue (utils/option.py)."""
    plan = Plan(int(B), int(H), int(W))
    on = np.ones(plan.B, bool)
    if np.random.rand() < 0.5:
        ms, rows, cols = [], [], []
        for _ in range(plan.B):
            m, R, C_ = warp_from_points(_draw_warp_points(plan.H, plan.W, args.proj), plan.H, plan.W)
            ms.append(m), rows.append(R), cols.append(C_)
        plan.warp = WarpPlan(np.stack(ms), np.array(rows, np.int32), np.array(cols, np.int32), on.copy())
    if np.random.rand() < 0.5:
        kernel_h = _randint(1, args.dila_ero_max_kernel + 1)
        kernel_w = _randint(1, args.dila_ero_max_kernel + 1)
        erode = _randint(0, 2) == 0
        # the element is np.ones((kernel_w, kernel_h)): the reference's kernel_w counts ROWS
        plan.morph = MorphPlan(kernel_w, kernel_h, int(args.dila_ero_iter), not erode, on.copy())
    if np.random.rand() < 0.5:
        jb, jc, js, jh = args.jitter_brightness, args.jitter_contrast, args.jitter_saturation, args.jitter_hue
        bs, cs, first = [], [], []
        for _ in range(plan.B):
            perm = torch.randperm(4).tolist()
            bs.append(_uniform(jb, max(0.0, 1.0 - jb), 1.0 + jb))
            cs.append(_uniform(jc, max(0.0, 1.0 - jc), 1.0 + jc))
            _uniform(js, max(0.0, 1.0 - js), 1.0 + js)      # saturation: an identity on a grey image, drawn all the same
            _uniform(jh, -jh, jh)                           # hue: returns a grey image as it is
            first.append(perm.index(1) < perm.index(0))
        plan.jitter = JitterPlan(np.array(bs, np.float32), np.array(cs, np.float32), np.array(first, bool), on.copy())
    validate_plan(plan)
    return plan


def validate_plan(plan: Plan):
    """every refusal that depends on the plan, on the host (nothing is launched): geometry and the caps of
    include/htrvt.h, the morphology's effective extent, the sigma of the left-out anti-aliasing filter"""
    B, H, W = plan.B, plan.H, plan.W
    if not (1 <= B <= MAX_B and 1 <= H <= MAX_H and 1 <= W <= MAX_W):
        raise ValueError(f"augment: batch {B} x {H} x {W} outside the caps (B <= {MAX_B}, H <= {MAX_H}, W <= {MAX_W})")
    for name, st in (("warp", plan.warp), ("morph", plan.morph), ("jitter", plan.jitter)):
        if st is not None and np.shape(st.on) != (B,):
            raise ValueError(f"augment: the {name} stage's on flags must have shape ({B},), got {np.shape(st.on)}")
    w = plan.warp
    if w is not None:
        if np.shape(w.m) != (B, 3, 3) or np.shape(w.rows) != (B,) or np.shape(w.cols) != (B,):
            raise ValueError(f"augment: warp plan needs m [{B},3,3], rows [{B}], cols [{B}]")
        for b in np.nonzero(w.on)[0]:
            R, C_ = int(w.rows[b]), int(w.cols[b])
            if not (1 <= R <= 2 * MAX_H and 1 <= C_ <= 2 * MAX_W) or not np.isfinite(w.m[b]).all():
                raise ValueError(f"augment: warp of image {b}: warped shape {R} x {C_} outside 1 .. {2 * MAX_H} x 1 .. {2 * MAX_W}, "
                                 "or a map that is not finite")
            sr, sc = max(0.0, (R / H - 1) / 2), max(0.0, (C_ / W - 1) / 2)
            if max(sr, sc) > MAX_SIGMA:
                raise ValueError(f"augment: warp of image {b}: the {R} x {C_} warped image shrinks to {H} x {W} with an anti-aliasing "
                                 f"sigma of {max(sr, sc):.3f}; the kernel leaves that filter out and serves sigma <= {MAX_SIGMA} "
                                 "only (a smaller --proj, or a taller image)")
    mp = plan.morph
    if mp is not None:
        if mp.rows < 1 or mp.cols < 1 or mp.iterations < 1:
            raise ValueError(f"augment: morphology needs rows, cols, iterations >= 1, got {mp.rows}, {mp.cols}, {mp.iterations}")
        re, ce = (mp.rows - 1) * mp.iterations + 1, (mp.cols - 1) * mp.iterations + 1
        if max(re, ce) > MAX_EXTENT:
            raise ValueError(f"augment: morphology element {mp.rows} x {mp.cols} over {mp.iterations} iterations has an effective "
                             f"extent of {re} x {ce}; at most {MAX_EXTENT} is served")
    j = plan.jitter
    if j is not None:
        if any(np.shape(a) != (B,) for a in (j.brightness, j.contrast, j.contrast_first)):
            raise ValueError(f"augment: jitter plan needs brightness, contrast, contrast_first of shape ({B},)")
        f = np.concatenate([np.asarray(j.brightness)[np.asarray(j.on, bool)], np.asarray(j.contrast)[np.asarray(j.on, bool)]])
        if np.isinf(f).any() or (f < 0).any():
            raise ValueError("augment: jitter factors must be finite and >= 0 (NaN = the step does not act)")


def _check_images(images, plan):
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise ValueError("augment: images must be a device (cuda) tensor; nothing runs on the host")
    if images.dtype != torch.uint8:
        raise ValueError(f"augment: images must be uint8, got {images.dtype}")
    if images.dim() != 4 or images.shape[1] != 1 or tuple(images.shape) != (plan.B, 1, plan.H, plan.W):
        raise ValueError(f"augment: images must be [B,1,H,W] = [{plan.B},1,{plan.H},{plan.W}] as the plan was drawn, got "
                         f"{tuple(images.shape)}")
    return images.contiguous()


def _to_device(arr, device):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(device)


def _warp(src, dst, plan):
    w = plan.warp
    tab = np.zeros(plan.B, _WARP_DT)
    tab["m"] = np.asarray(w.m, np.float64).reshape(plan.B, 9)
    tab["rows"], tab["cols"], tab["on"] = w.rows, w.cols, np.asarray(w.on, bool)
    t = _to_device(tab, src.device)
    check(lib.htrvt_aug_warp(ptr(src), ptr(t), ptr(dst), plan.B, plan.H, plan.W, stream()), "aug_warp")


def _morph(src, dst, plan):
    mp = plan.morph
    t = _to_device(np.asarray(mp.on, bool).astype(np.int32), src.device)
    check(lib.htrvt_aug_morph(ptr(src), ptr(t), ptr(dst), plan.B, plan.H, plan.W, mp.rows, mp.cols, mp.iterations, int(bool(mp.dilate)),
                              stream()), "aug_morph")


def _jitter(src, dst, plan):
    j = plan.jitter
    b, c = np.asarray(j.brightness, np.float32), np.asarray(j.contrast, np.float32)
    tab = np.zeros(plan.B, _JITTER_DT)
    tab["brightness"], tab["contrast"] = np.nan_to_num(b, nan=1.0), np.nan_to_num(c, nan=1.0)
    tab["flags"] = (ON * np.asarray(j.on, bool) + BRIGHTNESS * ~np.isnan(b) + CONTRAST * ~np.isnan(c)
                    + CONTRAST_FIRST * np.asarray(j.contrast_first, bool))
    t = _to_device(tab, src.device)
    check(lib.htrvt_aug_jitter(ptr(src), ptr(t), ptr(dst), plan.B, plan.H, plan.W, stream()), "aug_jitter")


_STAGES = (("warp", _warp), ("morph", _morph), ("jitter", _jitter))


def apply_plan(images_u8, plan: Plan):
    """device uint8 [B,1,H,W] -> device uint8 [B,1,H,W]: the stages of the plan, in the reference's order, on the current
    stream.  The input is never written; a plan with no stage returns it as it is."""
    validate_plan(plan)
    cur = _check_images(images_u8, plan)
    bufs = []
    with torch.cuda.device(cur.device):
        for name, run in _STAGES:
            if getattr(plan, name) is None:
                continue
            if len(bufs) < 2:
                bufs.append(torch.empty_like(cur))
            dst = bufs[0] if cur is not bufs[0] else bufs[1]
            run(cur, dst, plan)
            cur = dst
    return cur


def _single(images_u8, B, H, W, **stage):
    return apply_plan(images_u8, Plan(B, H, W, **stage))


def _on(on, B):
    return np.ones(B, bool) if on is None else np.asarray(on, bool)


def warp(images_u8, m, rows, cols, on=None):
    """the warp stage alone: m [B,3,3] float64, rows / cols [B] (shape of each warped image), on [B] (None: all)"""
    B, _, H, W = images_u8.shape
    return _single(images_u8, B, H, W, warp=WarpPlan(np.asarray(m, np.float64), np.asarray(rows, np.int32), np.asarray(cols, np.int32),
                                                     _on(on, B)))


def morph(images_u8, rows, cols, iterations=1, dilate=False, on=None):
    """the morphology stage alone: cv2.erode / cv2.dilate with np.ones((rows, cols)), `iterations` times"""
    B, _, H, W = images_u8.shape
    return _single(images_u8, B, H, W, morph=MorphPlan(int(rows), int(cols), int(iterations), bool(dilate), _on(on, B)))


def jitter(images_u8, brightness, contrast, contrast_first, on=None):
    """the jitter stage alone: per-image factors [B] (NaN: that step does not act), contrast_first [B]"""
    B, _, H, W = images_u8.shape
    return _single(images_u8, B, H, W, jitter=JitterPlan(np.asarray(brightness, np.float32), np.asarray(contrast, np.float32),
                                                         np.asarray(contrast_first, bool), _on(on, B)))


def SameTrCollate(batch, args, device="cuda"):
    """Drop-in for data/dataset.py:13-45 as a DataLoader collate_fn (functools.partial(SameTrCollate, args=args)).
    batch: [(image float [1,H,W] in 0 .. 1, label)].  Returns (uint8 device tensor [B,1,H,W], labels): the batch the model
    reads as value / 255, which is the reference's float batch.  It initialises the GPU, so it runs in the main process
    (--num-workers 0); a loader with workers calls draw_plan in the worker and apply_plan in the main process."""
    if torch.utils.data.get_worker_info() is not None:
        raise RuntimeError("htrvt_amd.SameTrCollate initialises the GPU and cannot run inside a DataLoader worker: use "
                           "num_workers=0, or call augment.draw_plan in the worker and augment.apply_plan in the main process")
    images, labels = zip(*batch)
    u8 = np.stack([np.uint8(np.asarray(im)[0] * 255) for im in images])[:, None]      # dataset.py:16
    plan = draw_plan(u8.shape[0], u8.shape[2], u8.shape[3], args)
    dev = torch.from_numpy(np.ascontiguousarray(u8)).to(torch.device(device))
    return apply_plan(dev, plan), labels
