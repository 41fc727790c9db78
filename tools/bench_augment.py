#!/usr/bin/env python3
"""Times of the train-time augmentation at B = 128, 64 x 1024, every stage forced on, one JSON line per leg:
  device    the three launches (htrvt_aug_warp / _morph / _jitter through the C entry points, tables already on the device)
            and apply_plan as SameTrCollate issues it (table upload included), device events after warm-up, two rounds
            alternated
  host      tests/augment_refs.py -- the numpy restatement of the reference's host pipeline -- over the same batch on one
            core, wall clock, once.  Not the reference's own time: skimage, cv2 and torchvision are not installed; the
            restatement does the same arithmetic per pixel in vectorised numpy.
The device result of the timed plan is checked against the host result before anything is printed.
    python tools/bench_augment.py [--iters 200] [--batch 128] [--host-images 128]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters, warm=10):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--host-images", type=int, default=128, help="images of the batch the host leg processes")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_augment.py measures on an MI355X: no GPU found")
    import augment_refs as A
    from htrvt_amd import augment
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import ptr, stream

    B, H, W = a.batch, 64, 1024
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
    np.random.seed(0)
    torch.manual_seed(0)
    pts = [augment._draw_warp_points(H, W, 8) for _ in range(B)]
    recs = [augment.warp_from_points(p, H, W) for p in pts]
    on = np.ones(B, bool)
    fb = rng.uniform(0.6, 1.4, B).astype(np.float32)
    fc = rng.uniform(0.6, 1.4, B).astype(np.float32)
    first = rng.integers(0, 2, B).astype(bool)
    plan = augment.Plan(B, H, W,
                        warp=augment.WarpPlan(np.stack([r[0] for r in recs]), np.array([r[1] for r in recs], np.int32),
                                              np.array([r[2] for r in recs], np.int32), on),
                        morph=augment.MorphPlan(3, 3, 1, False, on),
                        jitter=augment.JitterPlan(fb, fc, first, on))
    d = torch.from_numpy(x)[:, None].cuda()
    out = augment.apply_plan(d, plan)[:, 0].cpu().numpy()

    # the C entry points alone, on tables that are already on the device
    wt = np.zeros(B, augment._WARP_DT)
    wt["m"], wt["rows"], wt["cols"], wt["on"] = plan.warp.m.reshape(B, 9), plan.warp.rows, plan.warp.cols, 1
    jt = np.zeros(B, augment._JITTER_DT)
    jt["brightness"], jt["contrast"] = fb, fc
    jt["flags"] = augment.ON + augment.BRIGHTNESS + augment.CONTRAST + augment.CONTRAST_FIRST * first
    wt_d, jt_d = augment._to_device(wt, d.device), augment._to_device(jt, d.device)
    on_d = torch.ones(B, dtype=torch.int32, device="cuda")
    t0, t1 = torch.empty_like(d), torch.empty_like(d)
    legs = {
        "warp": lambda: check(lib.htrvt_aug_warp(ptr(d), ptr(wt_d), ptr(t0), B, H, W, stream())),
        "morph": lambda: check(lib.htrvt_aug_morph(ptr(t0), ptr(on_d), ptr(t1), B, H, W, 3, 3, 1, 0, stream())),
        "jitter": lambda: check(lib.htrvt_aug_jitter(ptr(t1), ptr(jt_d), ptr(t0), B, H, W, stream())),
        "apply_plan": lambda: augment.apply_plan(d, plan),
    }
    res = {}
    for _ in range(2):
        for name, fn in legs.items():
            res.setdefault(name, []).append(round(timed(fn, a.iters), 1))
    best = {k: min(v) for k, v in res.items()}

    n = min(a.host_images, B)
    ref = {"warp": None, "morph": (3, 3, 1, False), "jitter": None}
    ref["warp"] = [(r[0], r[1], r[2], None) for r in recs[:n]]
    ref["jitter"] = [(float(fb[i]), float(fc[i]), bool(first[i])) for i in range(n)]
    t = time.perf_counter()
    want, _ = A.collate(x[:n], ref)
    host_s = time.perf_counter() - t
    diff = np.abs(out[:n].astype(int) - want.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() <= 0.01, ("device and host results differ", int(diff.max()), float((diff > 0).mean()))

    print(json.dumps({"leg": "device", "B": B, "H": H, "W": W, "us": res, "three_launches_us": round(sum(best[k] for k in
                      ("warp", "morph", "jitter")), 1), "images_per_s_apply_plan": round(B / best["apply_plan"] * 1e6)}), flush=True)
    print(json.dumps({"leg": "host", "images": n, "H": H, "W": W, "seconds": round(host_s, 3), "ms_per_image": round(host_s / n * 1e3, 2),
                      "images_per_s_one_core": round(n / host_s, 1), "pixels_that_differ_from_device": int((diff > 0).sum()),
                      "note": "numpy restatement (tests/augment_refs.py), not the reference's skimage / cv2 / torchvision"}), flush=True)


if __name__ == "__main__":
    main()
