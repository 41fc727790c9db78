"""numpy restatements of the train-time augmentation (include/htrvt.h, htrvt_aug_*): the three stages of the
reference's collate function and its draw order, written from the behaviour of the libraries it calls (skimage's warp and
resize, cv2's erode / dilate, Pillow's blend under torchvision's ColorJitter) -- not from the kernels and not from those
libraries' text.  float64 and integers; no GPU is needed.  tests/test_augment_cpu.py pins this module to the installed
Pillow and scipy; tests/test_augment_gpu.py holds the kernels against it."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------------------- warp
def bilinear(a, b, c, d, dr, dc):
    return (1.0 - dr) * ((1.0 - dc) * a + dc * b) + dr * ((1.0 - dc) * c + dc * d)


def warp_stage(img, m, R, C):
    """skimage.transform.warp(img, m, output_shape=(R, C), order=1, mode='constant', cval=255, preserve_range=True): pixel
    (r, c) of the result is the source at m (c, r, 1), bilinear, every tap outside the image = 255.  float64 [R][C]."""
    H, W = img.shape
    src = np.full((H + 2, W + 2), 255.0)
    src[1:-1, 1:-1] = img
    r, c = np.mgrid[0:R, 0:C].astype(np.float64)
    with np.errstate(all="ignore"):
        u = m[0, 0] * c + m[0, 1] * r + m[0, 2]
        v = m[1, 0] * c + m[1, 1] * r + m[1, 2]
        q = m[2, 0] * c + m[2, 1] * r + m[2, 2]
        sc, sr = u / q, v / q
        far = ~((np.abs(sc) < 1e9) & (np.abs(sr) < 1e9))
    sc, sr = np.where(far, -5.0, sc), np.where(far, -5.0, sr)
    fr, fc = np.floor(sr), np.floor(sc)
    dr, dc = sr - fr, sc - fc

    def tap(rr, cc):          # index into the image framed with one ring of 255; anything further out is 255 too
        rr, cc = rr.astype(np.int64) + 1, cc.astype(np.int64) + 1
        inside = (rr >= 0) & (rr < H + 2) & (cc >= 0) & (cc < W + 2)
        return np.where(inside, src[np.clip(rr, 0, H + 1), np.clip(cc, 0, W + 1)], 255.0)

    out = bilinear(tap(fr, fc), tap(fr, fc + 1), tap(fr + 1, fc), tap(fr + 1, fc + 1), dr, dc)
    return np.where(far, 255.0, out)


def resize_stage(x, H, W):
    """skimage.transform.resize(x, (H, W), order=1, mode='reflect', anti_aliasing off): pixel centres at + 0.5, bilinear,
    indices clamped (= reflect for coordinates in (-1, size)).  float64 [H][W]."""
    R, C = x.shape
    rr = (np.arange(H) + 0.5) * (float(R) / float(H)) - 0.5
    cc = (np.arange(W) + 0.5) * (float(C) / float(W)) - 0.5
    fr, fc = np.floor(rr), np.floor(cc)
    dr, dc = (rr - fr)[:, None], (cc - fc)[None, :]
    r0, r1 = np.maximum(fr.astype(int), 0)[:, None], np.minimum(fr.astype(int) + 1, R - 1)[:, None]
    c0, c1 = np.maximum(fc.astype(int), 0)[None, :], np.minimum(fc.astype(int) + 1, C - 1)[None, :]
    return bilinear(x[r0, c0], x[r0, c1], x[r1, c0], x[r1, c1], dr, dc)


def warp(img, m, R, C):
    """RandomTransform.__call__ after its draws: warp to R x C, resize back, .astype(np.uint8) (toward zero)"""
    H, W = img.shape
    return np.clip(resize_stage(warp_stage(img, np.asarray(m, np.float64), int(R), int(C)), H, W), 0.0, 255.0).astype(np.uint8)


def solve_homography(src, dst):
    """m with m (src_i, 1) ~ (dst_i, 1), m[2,2] = 1, from the eight linear equations"""
    rows, rhs = [], []
    for (x, y), (u, v) in zip(src, dst):
        rows += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        rhs += [u, v]
    return np.append(np.linalg.solve(np.array(rows, np.float64), np.array(rhs, np.float64)), 1.0).reshape(3, 3)


# ------------------------------------------------------------------------------------------------------------ morph
def morph(img, rows, cols, iterations=1, dilate=False):
    """cv2.erode / cv2.dilate(img, np.ones((rows, cols)), iterations=...): anchor (rows // 2, cols // 2), the same offsets
    for both, pixels outside the image ignored; `iterations` passes one after the other (the kernel runs one wider pass)"""
    ay, ax = rows // 2, cols // 2
    H, W = img.shape
    neutral = 0 if dilate else 255
    out = img
    for _ in range(iterations):
        framed = np.full((H + rows - 1, W + cols - 1), neutral, np.uint8)
        framed[ay:ay + H, ax:ax + W] = out
        shifts = [framed[i:i + H, j:j + W] for i in range(rows) for j in range(cols)]
        out = np.max(shifts, 0) if dilate else np.min(shifts, 0)
    return out


# ----------------------------------------------------------------------------------------------------------- jitter
def blend(deg, f, x):
    """Pillow's Image.blend(constant image deg, x, f) for 8-bit pixels: float32, a rounded product and a rounded sum"""
    f = np.float32(f)
    t = np.float32(deg) + f * (x.astype(np.int32) - int(deg)).astype(np.float32)
    assert t.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.int32).astype(np.uint8)


def brightness(x, f):         # ImageEnhance.Brightness: blend with black
    return blend(0, f, x)


def contrast(x, f):           # ImageEnhance.Contrast: blend with the constant image int(mean + 0.5)
    s, n = int(x.astype(np.int64).sum()), x.size
    return blend((2 * s + n) // (2 * n), f, x)


def jitter(x, b, c, contrast_first):
    """ColorJitter on a grey image after its draws: b, c = the factors (NaN / None: the step does not act); saturation and
    hue leave a grey image as it is"""
    steps = [(contrast, c), (brightness, b)] if contrast_first else [(brightness, b), (contrast, c)]
    for fn, f in steps:
        if f is not None and not np.isnan(f):
            x = fn(x, f)
    return x


# ------------------------------------------------------------------------------------------------------------- plan
def draw_plan(B, H, W, args):
    """the collate function's draws, straight down the page: a dict of plain lists (None = the coin came up tails)"""
    out = {"warp": None, "morph": None, "jitter": None}
    if np.random.rand() < 0.5:
        out["warp"] = []
        for _ in range(B):
            horizontal = np.random.randint(0, 2) == 0
            dw, dh = (args.proj, 0) if horizontal else (0, args.proj)
            tl_top = np.random.uniform(-dh, dh)
            tl_left = np.random.uniform(-dw, dw)
            bl_bottom = np.random.uniform(-dh, dh)
            bl_left = np.random.uniform(-dw, dw)
            tr_top = np.random.uniform(-dh, dh)
            tr_right = np.random.uniform(-dw, min(W * 3 / 4 - tl_left, dw))
            br_bottom = np.random.uniform(-dh, dh)
            br_right = np.random.uniform(-dw, min(W * 3 / 4 - bl_left, dw))
            pts = [(tl_left, tl_top), (bl_left, H - bl_bottom), (W - br_right, H - br_bottom), (W - tr_right, tr_top)]
            m = solve_homography(pts, [(0, 0), (0, H - 1), (W - 1, H - 1), (W - 1, 0)])
            xs, ys = [p[0] for p in pts], [p[1] for p in pts]
            R, C = np.around((max(ys) - min(ys) + 1, max(xs) - min(xs) + 1))
            m = m @ np.array([[1.0, 0.0, min(xs)], [0.0, 1.0, min(ys)], [0.0, 0.0, 1.0]])
            out["warp"].append((m / m[2, 2], int(R), int(C), pts))
    if np.random.rand() < 0.5:
        kernel_h = int(torch.randint(1, args.dila_ero_max_kernel + 1, (1,)))
        kernel_w = int(torch.randint(1, args.dila_ero_max_kernel + 1, (1,)))
        erode = int(torch.randint(0, 2, (1,))) == 0
        out["morph"] = (kernel_w, kernel_h, args.dila_ero_iter, not erode)          # np.ones((kernel_w, kernel_h)): rows first
    if np.random.rand() < 0.5:
        out["jitter"] = []
        for _ in range(B):
            order = torch.randperm(4).tolist()
            f = []
            for v, lo, hi in [(args.jitter_brightness, None, None), (args.jitter_contrast, None, None),
                              (args.jitter_saturation, None, None), (args.jitter_hue, -args.jitter_hue, args.jitter_hue)]:
                lo, hi = (max(0.0, 1.0 - v), 1.0 + v) if lo is None else (lo, hi)
                f.append(float(torch.empty(1).uniform_(lo, hi)) if v != 0 else None)
            out["jitter"].append((f[0], f[1], order.index(1) < order.index(0)))
    return out


def collate(images_u8, plan):
    """the stages of a drawn plan (the dict above) over a uint8 batch [B][H][W]; returns the batch after each stage"""
    x = np.array(images_u8)
    stages = {}
    if plan["warp"] is not None:
        x = np.stack([warp(im, m, R, C) for im, (m, R, C, _) in zip(x, plan["warp"])])
        stages["warp"] = x
    if plan["morph"] is not None:
        rows, cols, it, dil = plan["morph"]
        x = np.stack([morph(im, rows, cols, it, dil) for im in x])
        stages["morph"] = x
    if plan["jitter"] is not None:
        x = np.stack([jitter(im, b, c, first) for im, (b, c, first) in zip(x, plan["jitter"])])
        stages["jitter"] = x
    return x, stages
