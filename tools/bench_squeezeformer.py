#!/usr/bin/env python3
"""The convolutional forks' GroupNorm mixer and squeeze-excite gate on one MI355X, at the forks' shapes: B = 128, C = 384
(ConvModule at dim 768), N = 128 (stage 1), 64 (stage 2) and 256, kernel 3, bfloat16 and float32; the SE gate at D = 768.
Forward and backward of the launch sequences seq_ops.gn_mixer_fwd / _bwd and seq_ops.se_fwd / _bwd (csrc/gnmixer.hip), and
beside each the same step composed from eager torch operators on the same device and dtype (GLU, conv1d on the transposed
rows, group_norm, silu; mean, two linears, the gate) with autograd for the backward.
Each leg is timed on its own: a warm-up, then `samples` windows of `reps` back-to-back calls between device events; the
median window is reported with the spread (min .. max), next to the leg's HBM floor -- the bytes its launches read and write,
each tensor once per launch that touches it, over 5.3 TB/s, the rate the project's HBM passes reach.  One JSON line per leg.
There is no speed gate.
    python tools/bench_squeezeformer.py [--reps 20] [--samples 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import htrvt_amd  # noqa: E402,F401
from htrvt_amd import seq_ops  # noqa: E402

HBM_BYTES_PER_US = 5.3e6


def timed_us(fn, reps, samples, warm=3):
    """(median, min, max) over `samples` windows of `reps` calls, microseconds per call"""
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


def report(leg, shape, dtype, nbytes, fn, fn_eager, args):
    t, lo, hi = timed_us(fn, args.reps, args.samples)
    te = timed_us(fn_eager, args.reps, args.samples)[0]
    floor = nbytes / HBM_BYTES_PER_US
    print(json.dumps({"leg": leg, **shape, "dtype": str(dtype).split(".")[1], "us": round(t, 2), "us_min": round(lo, 2),
                      "us_max": round(hi, 2), "bytes": nbytes, "hbm_floor_us": round(floor, 2), "share_of_floor": round(floor / t, 3),
                      "eager_us": round(te, 2), "eager_over_hip": round(te / t, 2)}), flush=True)


def mixer_legs(B, N, C, k, dtype, args):
    dev, es, rows = torch.device("cuda"), torch.empty(0, dtype=dtype).element_size(), B * N
    g = torch.Generator(device="cuda").manual_seed(0)
    u = torch.randn(rows, 2 * C, device=dev, generator=g).to(dtype)
    ds = torch.randn(rows, C, device=dev, generator=g).to(dtype)
    w = torch.randn(C, 1, k, device=dev, generator=g) * 0.4
    bias, gamma, beta = [torch.randn(C, device=dev, generator=g) for _ in range(3)]
    saved = seq_ops.gn_mixer_fwd(u, w, bias, gamma, beta, B, N)[1]
    # forward: u in, c out; c in, s out.  backward: (ds, c) in; (u, c, ds) in, du out
    io_f = (2 * C + C + C + C) * rows * es
    io_b = (2 * C + 2 * C + C + C + 2 * C) * rows * es
    wc = w.to(dtype)

    def eager(u_):
        x = F.glu(u_.view(B, N, 2 * C).transpose(1, 2), dim=1)
        x = F.conv1d(x, wc, bias.to(dtype), padding=k // 2, groups=C)
        return F.silu(F.group_norm(x, 1, gamma.to(dtype), beta.to(dtype), 1e-5)).transpose(1, 2).reshape(rows, C)
    ur = u.clone().requires_grad_(True)

    def eager_bwd():
        ur.grad = None
        eager(ur).backward(ds)
    shape = {"B": B, "N": N, "C": C, "k": k}
    with torch.no_grad():
        report("gn_mixer_fwd", shape, dtype, io_f, lambda: seq_ops.gn_mixer_fwd(u, w, bias, gamma, beta, B, N), lambda: eager(u), args)
    report("gn_mixer_bwd", shape, dtype, io_b, lambda: seq_ops.gn_mixer_bwd(ds, u, w, gamma, beta, B, N, saved), eager_bwd, args)
    print(json.dumps({"note": "eager gn_mixer_bwd includes its own forward", **shape}), flush=True)


def se_legs(B, N, D, dtype, args):
    dev, es, rows, H = torch.device("cuda"), torch.empty(0, dtype=dtype).element_size(), B * N, max(8, D // 4)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(rows, D, device=dev, generator=g).to(dtype)
    dy = torch.randn(rows, D, device=dev, generator=g).to(dtype)
    w1, b1 = torch.randn(H, D, device=dev, generator=g) * D ** -0.5, torch.zeros(H, device=dev)
    w2, b2 = torch.randn(D, H, device=dev, generator=g) * H ** -0.5, torch.zeros(D, device=dev)
    saved = seq_ops.se_fwd(x, w1, b1, w2, b2, B, N)[1]
    io_f = 3 * D * rows * es            # x for the means; x in, y out
    io_b = 4 * D * rows * es            # (dy, x) in for dg; dy in, dx out

    def eager(x_):
        s = x_.view(B, N, D).float().mean(1)
        gate = torch.sigmoid(F.linear(F.silu(F.linear(s, w1, b1)), w2, b2))
        return (x_.view(B, N, D) * gate[:, None].to(dtype)).view(rows, D)
    xr = x.clone().requires_grad_(True)

    def eager_bwd():
        xr.grad = None
        eager(xr).backward(dy)
    shape = {"B": B, "N": N, "D": D, "hidden": H}
    with torch.no_grad():
        report("se_fwd", shape, dtype, io_f, lambda: seq_ops.se_fwd(x, w1, b1, w2, b2, B, N), lambda: eager(x), args)
    report("se_bwd", shape, dtype, io_b, lambda: seq_ops.se_bwd(dy, x, w1, w2, B, N, saved), eager_bwd, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args()
    for dtype in (torch.bfloat16, torch.float32):
        for N in (128, 64, 256):
            mixer_legs(args.batch, N, 384, 3, dtype, args)
        se_legs(args.batch, 128, 768, dtype, args)


if __name__ == "__main__":
    main()
