#!/usr/bin/env python3
"""Per-launch time of the table-driven relative-position attention (csrc/attn_relpos.hip) against the dense-bias route
(htrvt_relpos_bias_fwd + the BIAS flavour of csrc/attention.hip forward; its backward with float atomics into a dense
d(bias) + htrvt_relpos_bias_bwd), B = 128, h = 6, hd = 128.  One JSON line per shape.
    python tools/bench_relpos.py [--iters 50]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters      # us per call


def run(iters):
    import torch
    import htrvt_amd  # noqa: F401
    from htrvt_amd import variants as V
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import ptr, stream
    BF = 1
    B, h, hd = 128, 6, 128
    for N in (128, 256):
        P = N
        for ws, shift in ((0, 0), (16, 0), (16, 8)):
            D = h * hd
            qkv = (torch.randn(B * N, 3 * D, device="cuda") * 1.2).bfloat16()
            dout = torch.randn(B * N, D, device="cuda").bfloat16()
            table = torch.randn(2 * P - 1, h, device="cuda") * 0.5
            out = torch.empty(B * N, D, device="cuda", dtype=torch.bfloat16)
            dqkv = torch.empty_like(qkv)
            lse = torch.empty(B * h, N, device="cuda")
            delta = torch.empty_like(lse)
            dtable = torch.zeros_like(table)
            work = torch.empty(V.relpos_workspace_floats(B, N, h, P, ws, shift), device="cuda")
            bias = torch.empty(h, N, N, device="cuda")
            dbias = torch.zeros(h, N, N, device="cuda")
            sc = hd ** -0.5

            def t_fwd():
                check(lib.htrvt_attn_relpos_fwd(ptr(qkv), ptr(table), ptr(out), ptr(lse), B, N, h, hd, sc, P, ws, shift, BF,
                                                stream()), "relpos_fwd")

            def t_bwd():
                check(lib.htrvt_attn_relpos_bwd(ptr(qkv), ptr(table), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv),
                                                ptr(dtable), ptr(work), B, N, h, hd, sc, P, ws, shift, BF, stream()), "relpos_bwd")

            def d_fwd():
                check(lib.htrvt_relpos_bias_fwd(ptr(table), ptr(bias), N, P, ws, shift, h, N, stream()), "bias_fwd")
                check(lib.htrvt_attn_fwd(ptr(qkv), ptr(bias), ptr(out), ptr(lse), B, N, h, hd, sc, BF, stream()), "attn_fwd")

            def d_bwd():
                dbias.zero_()
                check(lib.htrvt_attn_bwd(ptr(qkv), ptr(bias), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), ptr(dbias),
                                         B, N, h, hd, sc, BF, stream()), "attn_bwd")
                check(lib.htrvt_relpos_bias_bwd(ptr(dbias), ptr(dtable), N, P, ws, shift, h, N, stream()), "bias_bwd")

            t_fwd()
            r = dict(B=B, N=N, h=h, hd=hd, window=ws, shift=shift,
                     table_fwd_us=round(timed(t_fwd, iters), 1), table_bwd_us=round(timed(t_bwd, iters), 1))
            d_fwd()
            r.update(dense_fwd_us=round(timed(d_fwd, iters), 1), dense_bwd_us=round(timed(d_bwd, iters), 1))
            r["bwd_ratio"] = round(r["table_bwd_us"] / r["dense_bwd_us"], 3)
            r["fwd_ratio"] = round(r["table_fwd_us"] / r["dense_fwd_us"], 3)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    run(ap.parse_args().iters)
