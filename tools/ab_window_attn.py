#!/usr/bin/env python3
"""A/B of the window attention kernels (csrc/lgp.hip, csrc/swin.hip) between two builds of libhtrvt_hip.so in one process,
the protocol of DESIGN "Cost of the window shift":
    python tools/ab_window_attn.py PARENT.so NEW.so [--skip-speed]
bits   every output of htrvt_attn_local_fwd/bwd, htrvt_attn_local_shift_fwd/bwd and htrvt_attn_win2d_fwd/bwd (out, dqkv, dpad,
       dtable_partial) must be torch.equal between the two builds, in float32 and bfloat16, at the KERNEL_SHAPES of
       tests/swin_cases.py and at N in {12, 20, 100} x window in {3, 12, 16} x shift in {0, 5} x hd in {64, 128}.
speed  the window launches of tools/bench_lgp.py's kernel leg and the six of tools/bench_swin.py, forward and backward,
       interleaved: 25 rounds of 20 launches per library between a pair of events, median / minimum per launch.  PARENT.so is
       loaded a second time from a copy, and the gap between the two parent medians is the resolution of the method: a launch
       is `within` when NEW's median lies within twice that gap of PARENT's.
One process, no settings changed.  A failing call ends the run; differing outputs are listed with their size and the exit
status is non-zero if any output differs or any launch is slower."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import htrvt_amd  # noqa: E402,F401
from htrvt_amd import _lib  # noqa: E402
from htrvt_amd.ops import dt, ptr, stream  # noqa: E402
from swin_cases import KERNEL_SHAPES  # noqa: E402

ROUNDS, LAUNCHES = 25, 20


def load(path):
    l = ctypes.CDLL(os.path.abspath(path))
    for name, (res, argt) in _lib.PROTOTYPES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = res, argt
    return l


def call(l, name, *args):
    rc = getattr(l, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {l.htrvt_last_error().decode()}")


def local_case(l, B, N, heads, hd, w, shift, dtype, seed):
    """out, dqkv, dpad of one 1-D case; shift None: the unshifted entry points"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = heads * hd
    qkv = torch.randn(B * N, 3 * D, device="cuda", generator=g).to(dtype)
    dout = torch.randn(B * N, D, device="cuda", generator=g).to(dtype)
    bias = torch.randn(3 * D, device="cuda", generator=g)
    out, dqkv = torch.full_like(dout, 7.0), torch.full_like(qkv, 7.0)
    dpad = torch.full((B, 2 * D), 7.0, device="cuda")
    tail = (hd ** -0.5, dt(dtype), stream())
    if shift is None:
        call(l, "htrvt_attn_local_fwd", ptr(qkv), ptr(bias), ptr(out), B, N, heads, hd, w, *tail)
        call(l, "htrvt_attn_local_bwd", ptr(qkv), ptr(bias), ptr(dout), ptr(dqkv), ptr(dpad), B, N, heads, hd, w, *tail)
    else:
        call(l, "htrvt_attn_local_shift_fwd", ptr(qkv), ptr(bias), ptr(out), B, N, heads, hd, w, shift, *tail)
        call(l, "htrvt_attn_local_shift_bwd", ptr(qkv), ptr(bias), ptr(dout), ptr(dqkv), ptr(dpad), B, N, heads, hd, w, shift,
             *tail)
    torch.cuda.synchronize()
    return {"out": out, "dqkv": dqkv, "dpad": dpad}


def win2d_case(l, shape, dtype, seed):
    B, H, W, heads, hd, wh, ww, sh, sw = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, M = heads * hd, B * H * W
    qkv = torch.randn(M, 3 * D, device="cuda", generator=g).to(dtype)
    dout = torch.randn(M, D, device="cuda", generator=g).to(dtype)
    table = torch.randn((2 * wh - 1) * (2 * ww - 1), heads, device="cuda", generator=g)
    out, dqkv = torch.full_like(dout, 7.0), torch.full_like(qkv, 7.0)
    part = torch.full((l.htrvt_attn_win2d_rows(B, H, W, heads, wh, ww), table.numel()), 7.0, device="cuda")
    geo = (B, H, W, heads, hd, wh, ww, sh, sw, hd ** -0.5, dt(dtype), stream())
    call(l, "htrvt_attn_win2d_fwd", ptr(qkv), ptr(table), ptr(out), *geo)
    call(l, "htrvt_attn_win2d_bwd", ptr(qkv), ptr(table), ptr(dout), ptr(dqkv), ptr(part), *geo)
    torch.cuda.synchronize()
    return {"out": out, "dqkv": dqkv, "dtable_partial": part}


def bits(parent, new):
    cases = []
    for dtype in (torch.float32, torch.bfloat16):
        for shape in KERNEL_SHAPES:
            cases.append((f"win2d {shape} {dtype}", lambda l, s=shape, d=dtype: win2d_case(l, s, d, 1)))
        for B, heads in ((1, 1), (2, 3)):
            for N in (12, 20, 100):
                for w in (3, 12, 16):
                    for hd in (64, 128):
                        for shift in (None, 0, 5):
                            if shift is not None and shift >= w:
                                continue        # refused by both builds: the shift lies inside the window
                            cases.append((f"local B={B} heads={heads} N={N} w={w} hd={hd} shift={shift} {dtype}",
                                          lambda l, a=(B, N, heads, hd, w, shift, dtype): local_case(l, *a, 2)))
    tensors, differ = 0, []
    for name, run in cases:
        a, b = run(parent), run(new)
        for k in a:
            tensors += 1
            if not torch.equal(a[k], b[k]):
                d = (a[k].double() - b[k].double()).abs()
                differ.append(name)
                print(json.dumps({"leg": "bits", "case": name, "tensor": k, "elements": int((d > 0).sum()), "of": d.numel(),
                                  "max_abs": float(d.max()), "max_of_tensor": float(a[k].double().abs().max())}), flush=True)
    print(json.dumps({"leg": "bits", "cases": len(cases), "tensors": tensors, "cases_that_differ": len(set(differ)),
                      "equal": not differ}), flush=True)
    return not differ


def speed(libs):
    bf, dti, st = torch.bfloat16, dt(torch.bfloat16), stream()
    g = torch.Generator(device="cuda").manual_seed(0)
    launches = []           # (name, [closure per library])
    B, N, heads, hd, w = 128, 256, 6, 128, 12
    D = heads * hd
    qkv = torch.randn(B * N, 3 * D, device="cuda", generator=g).to(bf)
    dout = torch.randn(B * N, D, device="cuda", generator=g).to(bf)
    bias = torch.randn(3 * D, device="cuda", generator=g)
    out, dqkv, dpad = torch.empty_like(dout), torch.empty_like(qkv), torch.empty(B, 2 * D, device="cuda")
    tail = (B, N, heads, hd, w, hd ** -0.5, dti, st)
    launches.append((f"attn_local_fwd N={N} w={w} hd={hd}",
                     [lambda l=l, a=(ptr(qkv), ptr(bias), ptr(out)) + tail: call(l, "htrvt_attn_local_fwd", *a) for l in libs]))
    launches.append((f"attn_local_bwd N={N} w={w} hd={hd}",
                     [lambda l=l, a=(ptr(qkv), ptr(bias), ptr(dout), ptr(dqkv), ptr(dpad)) + tail:
                      call(l, "htrvt_attn_local_bwd", *a) for l in libs]))
    keep = [qkv, dout, bias, out, dqkv, dpad]
    W = 128
    for H, hd, (wh, ww) in ((4, 32, (4, 8)), (2, 64, (2, 8)), (1, 128, (1, 8))):
        D, M = heads * hd, B * H * W
        qkv = torch.randn(M, 3 * D, device="cuda", generator=g).to(bf)
        dout = torch.randn(M, D, device="cuda", generator=g).to(bf)
        table = torch.randn((2 * wh - 1) * (2 * ww - 1), heads, device="cuda", generator=g)
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        part = torch.empty(libs[0].htrvt_attn_win2d_rows(B, H, W, heads, wh, ww), table.numel(), device="cuda")
        keep += [qkv, dout, table, out, dqkv, part]
        for sh, sw in ((0, 0), (wh // 2, ww // 2)):
            geo = (B, H, W, heads, hd, wh, ww, sh, sw, hd ** -0.5, dti, st)
            tag = f"{H}x{W} {wh}x{ww} hd={hd} shift=({sh},{sw})"
            launches.append((f"win2d_fwd {tag}", [lambda l=l, a=(ptr(qkv), ptr(table), ptr(out)) + geo:
                                                  call(l, "htrvt_attn_win2d_fwd", *a) for l in libs]))
            launches.append((f"win2d_bwd {tag}", [lambda l=l, a=(ptr(qkv), ptr(table), ptr(dout), ptr(dqkv), ptr(part)) + geo:
                                                  call(l, "htrvt_attn_win2d_bwd", *a) for l in libs]))
    print("| launch | parent | parent again | this build | verdict |\n|---|---:|---:|---:|---|")
    worst = 0
    for name, fns in launches:
        for fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = [[] for _ in fns]
        for _ in range(ROUNDS):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LAUNCHES):
                    fn()
                e1.record()
                e1.synchronize()
                us[i].append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
        med, low = [statistics.median(u) for u in us], [min(u) for u in us]
        gap, delta = abs(med[1] - med[0]), med[2] - med[0]
        verdict = "within" if abs(delta) <= 2 * gap else ("faster" if delta < 0 else "slower")
        worst += verdict == "slower"
        print(f"| `{name}` | " + " | ".join(f"{m:.2f} / {lo:.2f} us" for m, lo in zip(med, low)) + f" | {verdict} |", flush=True)
        print(json.dumps({"leg": "speed", "launch": name, "median_us": [round(m, 3) for m in med],
                          "min_us": [round(m, 3) for m in low], "gap_us": round(gap, 3), "delta_us": round(delta, 3),
                          "verdict": verdict}), flush=True)
    del keep
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--skip-speed", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        again = shutil.copy(args.parent, os.path.join(tmp, "parent_again.so"))    # a second, independent load of the parent
        parent, parent2, new = load(args.parent), load(again), load(args.new)
        equal = bits(parent, new)
        slower = 0 if args.skip_speed else speed([parent, parent2, new])
    sys.exit(0 if equal and not slower else 1)


if __name__ == "__main__":
    main()
