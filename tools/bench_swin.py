#!/usr/bin/env python3
"""The Swin fork's window attention on one MI355X, bfloat16, at the fork's three stage shapes (B = 128, 6 heads): the 4 x 128
map with 4 x 8 windows and heads of 32, the 2 x 128 map with 2 x 8 windows and heads of 64, the 1 x 128 map with 1 x 8
windows and heads of 128, each unshifted and shifted by half a window.  Forward and backward of csrc/swin.hip, each timed
on its own (device events around `reps` back-to-back launches after a warm-up) and printed as a share of its HBM floor: the
tensor bytes read once and written once over the measured copy bandwidth of 6.3 TB/s -- forward: qkv in, out out; backward:
qkv and dout in, dqkv and the partial rows of the table gradient out.  One JSON line per leg.
    python tools/bench_swin.py [--reps 30]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import htrvt_amd  # noqa: E402,F401
from htrvt_amd._lib import check, lib  # noqa: E402
from htrvt_amd.ops import dt, ptr, stream  # noqa: E402

HBM_BYTES_PER_US = 6.3e6        # 6.3 TB/s: the measured float4-copy bandwidth, not the 8 TB/s of the data sheet


def timed_us(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--heads", type=int, default=6)
    args = ap.parse_args()
    B, W, heads, dtype = args.batch, args.width, args.heads, torch.bfloat16
    dev, dti, st, es = torch.device("cuda"), dt(dtype), stream(), 2
    g = torch.Generator(device="cuda").manual_seed(0)
    for H, hd, (wh, ww) in ((4, 32, (4, 8)), (2, 64, (2, 8)), (1, 128, (1, 8))):
        D, rows_tok = heads * hd, B * H * W
        qkv = torch.randn(rows_tok, 3 * D, device=dev, generator=g).to(dtype)
        dout = torch.randn(rows_tok, D, device=dev, generator=g).to(dtype)
        table = torch.randn((2 * wh - 1) * (2 * ww - 1), heads, device=dev, generator=g)
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        rows = lib.htrvt_attn_win2d_rows(B, H, W, heads, wh, ww)
        part = torch.empty(rows, table.numel(), device=dev)
        for sh, sw in ((0, 0), (wh // 2, ww // 2)):
            geo = (B, H, W, heads, hd, wh, ww, sh, sw, hd ** -0.5, dti, st)
            legs = [("win2d_fwd", (qkv.numel() + out.numel()) * es,
                     lambda: check(lib.htrvt_attn_win2d_fwd(ptr(qkv), ptr(table), ptr(out), *geo))),
                    ("win2d_bwd", (2 * qkv.numel() + dout.numel()) * es + part.numel() * 4,
                     lambda: check(lib.htrvt_attn_win2d_bwd(ptr(qkv), ptr(table), ptr(dout), ptr(dqkv), ptr(part), *geo)))]
            for leg, nbytes, fn in legs:
                t = timed_us(fn, args.reps)
                floor = nbytes / HBM_BYTES_PER_US
                print(json.dumps({"leg": leg, "B": B, "H": H, "W": W, "heads": heads, "hd": hd, "window": [wh, ww],
                                  "shift": [sh, sw], "us": round(t, 2), "bytes": nbytes, "hbm_floor_us": round(floor, 2),
                                  "share_of_floor": round(floor / t, 3)}), flush=True)
        del qkv, dout, out, dqkv, part


if __name__ == "__main__":
    main()
