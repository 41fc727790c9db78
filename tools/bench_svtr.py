#!/usr/bin/env python3
"""The SVTR fork's local attention on one MI355X, bfloat16, at the fork's three local maps (B = 128, heads of 32, the 7 x 11
box): 16 x 128 with 2 heads, 8 x 128 with 4 heads, 4 x 128 with 8 heads.  Forward and backward of csrc/svtr.hip, and beside
them the dense route the project had for the same result: the fused attention of csrc/attention.hip over all N = H W keys
with a float32 [heads, N, N] bias holding -30000 outside the box (htrvt_attn_fwd / _bwd).
Each leg is timed on its own: a warm-up, then `samples` windows of `reps` back-to-back launches between device events; the
median window is reported, with the spread (min .. max), as a share of the leg's HBM floor -- the tensor bytes read once and
written once over the measured copy bandwidth of 6.3 TB/s.  Forward: qkv in, out and lse out; backward: qkv, out, dout and
lse in, dqkv out.  The dense legs' floors count the bias too.  One JSON line per leg.
    python tools/bench_svtr.py [--reps 20] [--samples 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import htrvt_amd  # noqa: E402,F401
from htrvt_amd._lib import check, lib  # noqa: E402
from htrvt_amd.ops import dt, ptr, stream  # noqa: E402

HBM_BYTES_PER_US = 6.3e6        # 6.3 TB/s: the measured float4-copy bandwidth, not the 8 TB/s of the data sheet
MASKED = -30000.0               # exp underflows to exactly 0 in float32: the dense route's -inf


def timed_us(fn, reps, samples, warm=3):
    """(median, min, max) over `samples` windows of `reps` launches, microseconds per launch"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(out), min(out), max(out)


def box_bias(H, W, heads, kernel, dev):
    """float32 [heads, N, N]: 0 inside the box, MASKED outside"""
    y, x = torch.arange(H * W, device=dev) // W, torch.arange(H * W, device=dev) % W
    vis = ((y[:, None] - y[None, :]).abs() <= kernel[0] // 2) & ((x[:, None] - x[None, :]).abs() <= kernel[1] // 2)
    return torch.where(vis, 0.0, MASKED).float().expand(heads, -1, -1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense-bias legs")
    args = ap.parse_args()
    B, W, hd, (kh, kw), dtype = args.batch, args.width, 32, (7, 11), torch.bfloat16
    dev, dti, st, es = torch.device("cuda"), dt(dtype), stream(), 2
    g = torch.Generator(device="cuda").manual_seed(0)
    for H, heads in ((16, 2), (8, 4), (4, 8)):
        D, N, rows = heads * hd, H * W, B * H * W
        qkv = torch.randn(rows, 3 * D, device=dev, generator=g).to(dtype)
        dout = torch.randn(rows, D, device=dev, generator=g).to(dtype)
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        lse = torch.empty(B * heads, N, device=dev)
        geo = (B, H, W, heads, hd, kh, kw, hd ** -0.5, dti, st)
        io_f, io_b = (qkv.numel() + out.numel()) * es + lse.numel() * 4, (2 * qkv.numel() + 2 * dout.numel()) * es + lse.numel() * 4
        legs = [("nbr2d_fwd", io_f, lambda: check(lib.htrvt_attn_nbr2d_fwd(ptr(qkv), ptr(out), ptr(lse), *geo))),
                ("nbr2d_bwd", io_b, lambda: check(lib.htrvt_attn_nbr2d_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), *geo)))]
        if not args.no_dense:
            bias = box_bias(H, W, heads, (kh, kw), dev)
            out_d, lse_d, delta = torch.empty_like(out), torch.empty_like(lse), torch.empty_like(lse)
            dgeo = (B, N, heads, hd, hd ** -0.5, dti, st)
            check(lib.htrvt_attn_fwd(ptr(qkv), ptr(bias), ptr(out_d), ptr(lse_d), *dgeo))
            check(lib.htrvt_attn_nbr2d_fwd(ptr(qkv), ptr(out), ptr(lse), *geo))
            torch.cuda.synchronize()
            diff = float((out_d.float() - out.float()).abs().max())      # the two routes compute the same thing
            legs += [("dense_bias_fwd", io_f + bias.numel() * 4,
                      lambda: check(lib.htrvt_attn_fwd(ptr(qkv), ptr(bias), ptr(out_d), ptr(lse_d), *dgeo))),
                     ("dense_bias_bwd", io_b + bias.numel() * 4 + delta.numel() * 8,
                      lambda: check(lib.htrvt_attn_bwd(ptr(qkv), ptr(bias), ptr(out_d), ptr(dout), ptr(lse_d), ptr(delta), ptr(dqkv),
                                                       None, *dgeo)))]
        for leg, nbytes, fn in legs:
            t, lo, hi = timed_us(fn, args.reps, args.samples)
            floor = nbytes / HBM_BYTES_PER_US
            rec = {"leg": leg, "B": B, "H": H, "W": W, "heads": heads, "hd": hd, "kernel": [kh, kw], "us": round(t, 2),
                   "us_min": round(lo, 2), "us_max": round(hi, 2), "bytes": nbytes, "hbm_floor_us": round(floor, 2),
                   "share_of_floor": round(floor / t, 3)}
            if leg.startswith("dense"):
                rec["max_abs_diff_to_nbr2d"] = round(diff, 5)
            print(json.dumps(rec), flush=True)
        del qkv, dout, out, dqkv, lse


if __name__ == "__main__":
    main()
