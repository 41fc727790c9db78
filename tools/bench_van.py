#!/usr/bin/env python3
"""The VAN forks' depthwise convolutions and modules on one MI355X, bfloat16, at the forks' own map B = 128, H = 4,
W = 128, C = 768 (and the horizontal mixer's H = 1): every launch of the three depthwise forms -- 5x5, 7x7 dilation 3,
1x9 -- forward, input gradient and weight gradient, timed on its own (device events around `reps` back-to-back launches
after a warm-up) and printed as a share of its HBM floor: the tensor bytes read once and written once (from the shapes,
listed below) over the measured copy bandwidth of 6.3 TB/s.  Then VANHeightReducer and HorizontalMixer, forward and
forward + backward, next to a torch-eager restatement of the two modules written here from nn.Conv2d / nn.BatchNorm2d /
nn.GELU in channels-last bfloat16 on the same GPU.  One JSON line per leg.
One activation is 100 MB at H = 4 and 25 MB at H = 1, so the H = 1 launches can be served by the 256 MB Infinity Cache
and run below their HBM floor.
    python tools/bench_van.py [--reps 30] [--skip-eager]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import htrvt_amd  # noqa: E402,F401
from htrvt_amd import van  # noqa: E402
from htrvt_amd._lib import check, lib  # noqa: E402
from htrvt_amd.ops import colsum, dt, ptr, stream  # noqa: E402

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


class EagerBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj1, self.act = nn.Conv2d(dim, dim, 1), nn.GELU()
        self.dw = nn.Conv2d(dim, dim, 5, padding=2, groups=dim, bias=False)
        self.dwd = nn.Conv2d(dim, dim, 7, padding=9, dilation=3, groups=dim, bias=False)
        self.pw, self.bn = nn.Conv2d(dim, dim, 1, bias=False), nn.BatchNorm2d(dim)
        self.proj2, self.norm = nn.Conv2d(dim, dim, 1), nn.BatchNorm2d(dim)

    def forward(self, x):
        u = self.act(self.proj1(x))
        return x + self.norm(self.proj2(u * self.bn(self.pw(self.dwd(self.dw(u))))))


class EagerReducer(nn.Module):
    def __init__(self, dim, depth=2):
        super().__init__()
        self.blocks = nn.Sequential(*[EagerBlock(dim) for _ in range(depth)])

    def forward(self, x):
        return self.blocks(x).mean(2, keepdim=True)


class EagerMixer(nn.Module):
    def __init__(self, dim, k=9):
        super().__init__()
        self.dw = nn.Conv2d(dim, dim, (1, k), padding=(0, k // 2), groups=dim, bias=False)
        self.pw, self.bn, self.act = nn.Conv2d(dim, dim, 1, bias=False), nn.BatchNorm2d(dim), nn.GELU()

    def forward(self, x):
        return self.act(x + self.bn(self.pw(self.dw(x))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--skip-eager", action="store_true")
    args = ap.parse_args()
    B, W, C, dtype = args.batch, args.width, args.dim, torch.bfloat16
    dev, dti, st, es = torch.device("cuda"), dt(dtype), stream(), 2
    g = torch.Generator(device="cuda").manual_seed(0)

    # ---- the depthwise launches one by one
    for name, H, kh, kw, dil in (("5x5 d1", 4, 5, 5, 1), ("7x7 d3", 4, 7, 7, 3), ("1x9 d1", 1, 1, 9, 1)):
        x = torch.randn(B, H, W, C, device=dev, generator=g).to(dtype)
        dy = torch.randn(B, H, W, C, device=dev, generator=g).to(dtype)
        w = (torch.randn(C, kh * kw, device=dev, generator=g) * 0.2).contiguous()
        y = torch.empty_like(x)
        geo = (B, H, W, C, kh, kw, dil, dti)
        rows = lib.htrvt_van_dw_rows(*geo)
        part, dw = torch.empty(rows, C * kh * kw, device=dev), torch.zeros(C, kh * kw, device=dev)
        act = x.numel() * es
        legs = [
            ("dw_fwd", 2 * act, lambda: check(lib.htrvt_van_dw_fwd(ptr(x), ptr(w), ptr(y), *geo, st))),
            ("dw_bwd_input", 2 * act, lambda: check(lib.htrvt_van_dw_bwd_input(ptr(dy), ptr(w), None, ptr(y), *geo, st))),
            ("dw_bwd_input + add", 3 * act, lambda: check(lib.htrvt_van_dw_bwd_input(ptr(dy), ptr(w), ptr(x), ptr(y), *geo, st))),
            ("dw_bwd_weight", 2 * act + part.numel() * 4,       # reads x and dy, writes the partial rows
             lambda: check(lib.htrvt_van_dw_bwd_weight(ptr(x), ptr(dy), ptr(part), *geo, st))),
            ("colsum (d weight)", part.numel() * 4, lambda: colsum(part, rows, C * kh * kw, C * kh * kw, dw, dti=0)),
        ]
        for leg, nbytes, fn in legs:
            t = timed_us(fn, args.reps)
            floor = nbytes / HBM_BYTES_PER_US
            print(json.dumps({"leg": leg, "form": name, "B": B, "H": H, "W": W, "C": C, "us": round(t, 2), "bytes": nbytes,
                              "hbm_floor_us": round(floor, 2), "share_of_floor": round(floor / t, 3)}), flush=True)
        del x, dy, y, part

    # ---- the modules, and the eager restatement on the same GPU
    for name, H, hip, eager in (("VANHeightReducer", 4, lambda: van.VANHeightReducer(C, compute_dtype=dtype), lambda: EagerReducer(C)),
                                ("HorizontalMixer", 1, lambda: van.HorizontalMixer(C, compute_dtype=dtype), lambda: EagerMixer(C))):
        x = torch.randn(B, C, H, W, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, C, 1, W, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        res = {"leg": "module", "module": name, "B": B, "H": H, "W": W, "C": C}

        def legs_of(m, xin, dyin):
            xr = xin.clone().requires_grad_(True)

            def fwd():
                with torch.no_grad():
                    m(xin)

            def fwd_bwd():
                xr.grad = None
                for p in m.parameters():
                    p.grad = None
                m(xr).backward(dyin)
            return round(timed_us(fwd, args.reps), 1), round(timed_us(fwd_bwd, args.reps), 1)
        res["hip_fwd_us"], res["hip_fwd_bwd_us"] = legs_of(hip().to(dev).train(), x, dy)
        if not args.skip_eager:
            m = eager().to(dev).to(dtype).to(memory_format=torch.channels_last).train()
            res["eager_fwd_us"], res["eager_fwd_bwd_us"] = legs_of(m, x.to(dtype), dy.to(dtype))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
