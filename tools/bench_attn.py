#!/usr/bin/env python3
"""Time the fused attention kernels (csrc/attention.hip) at the model shapes, A/B in one process.
    python tools/bench_attn.py
    python tools/bench_attn.py --drop 0.05      what dropout on the probabilities costs: p = 0 and p interleaved"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import torch
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import ptr, stream
    shapes = [(128, 256, 6, 128), (64, 512, 6, 128), (128, 128, 6, 128), (256, 256, 8, 64)]
    for B, N, h, hd in shapes:
        D = h * hd
        qkv = (torch.randn(B * N, 3 * D, device="cuda") * 1.2).bfloat16()
        dout = torch.randn(B * N, D, device="cuda").bfloat16()
        out = torch.empty(B * N, D, device="cuda", dtype=torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        lse = torch.empty(B * h, N, device="cuda")
        delta = torch.empty_like(lse)
        sc = hd ** -0.5
        bias = dbias = None

        def fwd():
            check(lib.htrvt_attn_fwd(ptr(qkv), ptr(bias), ptr(out), ptr(lse), B, N, h, hd, sc, 1, stream()), "f")

        def bwd():
            check(lib.htrvt_attn_bwd(ptr(qkv), ptr(bias), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), ptr(dbias), B, N, h, hd, sc, 1, stream()), "b")

        res = []
        for fn, flops, byts in ((fwd, 4.0 * B * h * N * N * hd, 2 * B * N * 4 * D), (bwd, 14.0 * B * h * N * N * hd, 2 * B * N * 12 * D)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / 20 * 1e3
            res.append(f"{us:8.1f} us {flops / us / 1e6:7.1f} TF/s {byts / us / 1e6:5.2f} TB/s(min bytes)")
        print(f"B={B} N={N} h={h} hd={hd}: fwd {res[0]} | bwd(dq+dkv, 7 products) {res[1]}", flush=True)


def run_drop(p, rounds):
    """forward and backward at p = 0 (htrvt_attn_fwd/_bwd) and at p (htrvt_attn_dropout_*), `rounds` interleaved timings of
    20 launches each: the spread of the p = 0 rounds is the tool's run-to-run noise"""
    import torch
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops as S
    for B, N, h, hd in [(128, 256, 6, 128), (128, 128, 6, 128)]:
        D = h * hd
        qkv = (torch.randn(B * N, 3 * D, device="cuda") * 1.2).bfloat16()
        dout = torch.randn(B * N, D, device="cuda").bfloat16()
        seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
        state = {}

        def fwd(drop):
            state[drop is None] = S.attention_fwd(qkv, B, N, h, drop=drop)

        def bwd(drop):
            out, lse = state[drop is None]
            S.attention_bwd(qkv, out, dout, lse, B, N, h, drop=drop)

        times = {}
        for _ in range(rounds):
            for fn in (fwd, bwd):
                for drop in (None, (seed, p)):
                    for _ in range(3):
                        fn(drop)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn(drop)
                    e1.record()
                    torch.cuda.synchronize()
                    times.setdefault((fn.__name__, 0.0 if drop is None else p), []).append(e0.elapsed_time(e1) / 20 * 1e3)
        for (name, q), ts in times.items():
            ts = sorted(ts)
            print(f"B={B} N={N} h={h} hd={hd} {name} p={q}: median {ts[len(ts) // 2]:7.1f} us, min {ts[0]:7.1f}, max {ts[-1]:7.1f} "
                  f"over {rounds} rounds (host allocation included)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drop", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.drop > 0:
        run_drop(args.drop, args.rounds)
    else:
        run()
