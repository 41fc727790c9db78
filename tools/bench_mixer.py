#!/usr/bin/env python3
"""The convolutional token mixer's kernels on one MI355X at B = 128, N = 128, D = 768, k = 7, bfloat16: every launch of
seq_ops.conv_mixer_fwd / conv_mixer_bwd timed on its own (device events around `reps` back-to-back launches after a
warm-up) next to its HBM floor -- the bytes the launch must move (from the shapes, listed below) over the measured copy
bandwidth of 6.3 TB/s -- then the whole sequences, and next to them the ATen sequence (F.glu, conv1d(groups=D) on
[B, D, N], batch_norm, silu) for the same tensors on the same GPU.  One JSON line per leg.
The working set (u: 50 MB, c / s: 25 MB each) fits the 256 MB Infinity Cache, so a launch can run below its HBM floor.
    python tools/bench_mixer.py [--reps 50]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import htrvt_amd  # noqa: E402,F401
from htrvt_amd import seq_ops  # noqa: E402
from htrvt_amd._lib import check, lib  # noqa: E402
from htrvt_amd.ops import colsum, dt, ptr, stream  # noqa: E402

HBM_BYTES_PER_US = 6.3e6        # 6.3 TB/s: the measured float4-copy bandwidth, not the 8 TB/s of the data sheet


def timed_us(fn, reps, warm=5):
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--kernel-size", type=int, default=7)
    args = ap.parse_args()
    B, N, D, k, dtype = args.batch, args.tokens, args.dim, args.kernel_size, torch.bfloat16
    dev, dti, st, R, es = torch.device("cuda"), dt(dtype), stream(), B * N, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    u = torch.randn(R, 2 * D, device=dev, generator=g).to(dtype)
    ds = torch.randn(R, D, device=dev, generator=g).to(dtype)
    w = (torch.randn(D, 1, k, device=dev, generator=g) * 0.4).contiguous()
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    rm, rv, nbt = torch.zeros(D, device=dev), torch.ones(D, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    bn = (gamma, beta, rm, rv, nbt)
    shape = {"B": B, "N": N, "D": D, "k": k, "dtype": "bfloat16"}

    # ---- the launches one by one, on buffers of one train forward
    s, saved = seq_ops.conv_mixer_fwd(u, w, B, N, bn=bn, training=True)
    c, scale, shift, mean, rstd = saved
    rows = lib.htrvt_mixer_rows(B, N, D, dti)
    part = torch.empty(lib.htrvt_mixer_fwd_workspace_floats(B, N, D, dti), device=dev)
    q = lib.htrvt_mixer_reduce_rows(R, D, dti)
    qpart, coef = torch.empty(q, 2, D, device=dev), torch.empty(3, D, device=dev)
    dgb = torch.zeros(2, D, device=dev)
    pw, du, dw = torch.empty(rows, D * k, device=dev), torch.empty_like(u), torch.zeros(D, 1, k, device=dev)
    act = R * D * es          # bytes of one [B*N, D] activation
    legs = [
        ("mixer_fwd_train", 3 * act + rows * 2 * D * 4,        # reads u (2 act), writes c and the partial rows
         lambda: check(lib.htrvt_mixer_fwd_train(ptr(u), ptr(w), ptr(c), ptr(part), B, N, D, k, dti, st))),
        ("bn_finalize", rows * 2 * D * 4,
         lambda: check(lib.htrvt_bn_finalize(ptr(part), rows, D, float(R), ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(rm), ptr(rv),
                                             ptr(nbt), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), st))),
        ("mixer_bn_silu", 2 * act,                             # reads c, writes s
         lambda: check(lib.htrvt_mixer_bn_silu(ptr(c), ptr(scale), ptr(shift), ptr(s), R, D, dti, st))),
        ("mixer_fwd_eval", 3 * act,                            # reads u, writes s (no c: no backward follows)
         lambda: check(lib.htrvt_mixer_fwd_eval(ptr(u), ptr(w), ptr(scale), ptr(shift), None, ptr(s), B, N, D, k, dti, st))),
        ("mixer_bwd_reduce", 2 * act + q * 2 * D * 4,          # reads ds and c
         lambda: check(lib.htrvt_mixer_bwd_reduce(ptr(ds), ptr(c), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(qpart), R, D,
                                                  dti, st))),
        ("bn_bwd_finalize", q * 2 * D * 4,
         lambda: check(lib.htrvt_bn_bwd_finalize(ptr(qpart), q, D, float(R), ptr(gamma), ptr(mean), ptr(rstd), ptr(dgb[0]),
                                                 ptr(dgb[1]), ptr(coef), st))),
        ("mixer_bwd", 6 * act + rows * D * k * 4,              # reads u, c, ds (4 act), writes du (2 act) and the partial rows
         lambda: check(lib.htrvt_mixer_bwd(ptr(u), ptr(c), ptr(ds), ptr(w), ptr(scale), ptr(shift), ptr(coef), ptr(du), ptr(pw),
                                           None, B, N, D, k, dti, st))),
        ("colsum (d weight)", rows * D * k * 4,
         lambda: colsum(pw, rows, D * k, D * k, dw, dti=0)),
    ]
    for name, nbytes, fn in legs:
        t = timed_us(fn, args.reps)
        print(json.dumps({"leg": name, **shape, "us": round(t, 2), "bytes": nbytes,
                          "hbm_floor_us": round(nbytes / HBM_BYTES_PER_US, 2)}), flush=True)

    # ---- the sequences, and ATen's on the same tensors
    ur = u.clone().requires_grad_(True)
    wr, gr, br = w.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

    def hip_fwd():
        return seq_ops.conv_mixer_fwd(u, w, B, N, bn=bn, training=True)

    def hip_fwd_bwd():
        _, sv = hip_fwd()
        seq_ops.conv_mixer_bwd(ds, u, w, B, N, sv, gamma=gamma, training=True)

    def aten_fwd():
        y = F.glu(ur, dim=-1).view(B, N, D).transpose(1, 2)
        y = F.conv1d(y, wr.to(dtype), None, padding=k // 2, groups=D)
        y = F.batch_norm(y, rm, rv, gr, br, True, 0.1, 1e-5)
        return F.silu(y).transpose(1, 2).reshape(R, D)

    def aten_fwd_bwd():
        for t in (ur, wr, gr, br):
            t.grad = None
        aten_fwd().backward(ds)

    def aten_fwd_nograd():
        with torch.no_grad():
            aten_fwd()
    res = {"leg": "sequence", **shape,
           "hip_fwd_us": round(timed_us(hip_fwd, args.reps), 1), "aten_fwd_us": round(timed_us(aten_fwd_nograd, args.reps), 1),
           "hip_fwd_bwd_us": round(timed_us(hip_fwd_bwd, args.reps), 1),
           "aten_fwd_bwd_us": round(timed_us(aten_fwd_bwd, args.reps), 1),
           "fwd_hbm_floor_us": round(5 * act / HBM_BYTES_PER_US, 1), "fwd_bwd_hbm_floor_us": round(13 * act / HBM_BYTES_PER_US, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
