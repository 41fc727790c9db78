#!/usr/bin/env python3
"""The convolutional forks' GroupNorm mixer and squeeze-excite gate on one MI355X, at the forks' shapes: B = 128, C = 384
(ConvModule at dim 768), N = 128 (stage 1), 64 (stage 2) and 256, kernel 3, bfloat16 and float32; the SE gate at D = 768.
Forward and backward of the launch sequences seq_ops.gn_mixer_fwd / _bwd and seq_ops.se_fwd / _bwd (csrc/gnmixer.hip), and
beside each the same step composed from eager torch operators on the same device and dtype (GLU, conv1d on the transposed
rows, group_norm, silu; mean, two linears, the gate) with autograd for the backward.
Each leg is timed on its own: a warm-up, then `samples` windows of `reps` back-to-back calls between device events; the
median window is reported with the spread (min .. max), next to the leg's HBM floor -- the bytes its launches read and write,
each tensor once per launch that touches it, over 5.3 TB/s, the rate the project's HBM passes reach.  One JSON line per leg.
Two more legs are comparisons of two arms from the same build, in one process, their windows alternated sample by sample:
`dropnorm`, each kernel of csrc/dropnorm.hip against the two launches it replaces at [128 * 128, 768] (bytes over time per arm),
and `block_dropout`, a ConformerBlock's train step at (128, 128, 768) with the forks' rates against the same block with zero
rates.  There is no speed gate.
    python tools/bench_squeezeformer.py [--reps 20] [--samples 7] [--legs mixer,se,dropnorm,block_dropout]
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


def alternated_us(fns, reps, samples, warm=3):
    """[(median, min, max)] per function, microseconds per call: every sample times one window of `reps` calls of each
    function in turn, so that the arms of a comparison share the machine's state"""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(samples):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1) / reps * 1e3)
    return [(statistics.median(o), min(o), max(o)) for o in out]


def dropnorm_legs(rows, D, N, dtype, p, p_path, args):
    """csrc/dropnorm.hip against the two launches each kernel replaces, through the C ABI on preallocated buffers:
    forward  htrvt_drop_add_ln_fwd     vs htrvt_residual_dropout + htrvt_layernorm_fwd    (4 vs 5 tensor passes over [rows, D])
    backward htrvt_layernorm_bwd_drop  vs htrvt_layernorm_bwd + htrvt_residual_dropout    (5 vs 6)"""
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import dt, ptr, stream
    dev, es, dti = torch.device("cuda"), torch.empty(0, dtype=dtype).element_size(), dt(dtype)
    g = torch.Generator(device="cuda").manual_seed(0)
    x, res, dy, dres = [torch.randn(rows, D, device=dev, generator=g).to(dtype) for _ in range(4)]
    gamma, beta = torch.randn(D, device=dev, generator=g) + 1, torch.randn(D, device=dev, generator=g)
    seeds = torch.randint(0, 2 ** 62, (2,), dtype=torch.int64, device=dev, generator=g)
    s, y, ds, dxb = [torch.empty_like(x) for _ in range(4)]
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    partial = torch.empty(lib.htrvt_layernorm_bwd_blocks(rows), 2, D, device=dev)
    st = stream()

    def fwd_fused():
        check(lib.htrvt_drop_add_ln_fwd(ptr(x), ptr(res), ptr(seeds), p, p_path, N, ptr(gamma), ptr(beta), ptr(s), ptr(y), ptr(mean),
                                        ptr(rstd), rows, D, 1e-6, dti, st))

    def fwd_pair():
        check(lib.htrvt_residual_dropout(ptr(x), ptr(res), ptr(s), N, rows * D, D, ptr(seeds), p, p_path, dti, st))
        check(lib.htrvt_layernorm_fwd(ptr(s), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, D, 1e-6, dti, st))

    def bwd_fused():
        check(lib.htrvt_layernorm_bwd_drop(ptr(dy), ptr(s), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(seeds), p, p_path, N,
                                           ptr(ds), ptr(dxb), ptr(partial), rows, D, dti, st))

    def bwd_pair():
        check(lib.htrvt_layernorm_bwd(ptr(dy), ptr(s), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(ds), ptr(partial), rows, D,
                                      dti, st))
        check(lib.htrvt_residual_dropout(ptr(ds), None, ptr(dxb), N, rows * D, D, ptr(seeds), p, p_path, dti, st))
    fwd_fused()
    one = rows * D * es
    for leg, fused, pair, nf, npair in (("dropnorm_fwd", fwd_fused, fwd_pair, 4, 5), ("dropnorm_bwd", bwd_fused, bwd_pair, 5, 6)):
        (tf, fl, fh), (tp, pl, ph) = alternated_us([fused, pair], args.reps, args.samples)
        print(json.dumps({"leg": leg, "rows": rows, "D": D, "dtype": str(dtype).split(".")[1], "p": p, "p_path": p_path,
                          "fused_us": round(tf, 2), "fused_min": round(fl, 2), "fused_max": round(fh, 2),
                          "pair_us": round(tp, 2), "pair_min": round(pl, 2), "pair_max": round(ph, 2),
                          "fused_bytes": nf * one, "pair_bytes": npair * one, "fused_TBps": round(nf * one / tf / 1e6, 3),
                          "pair_TBps": round(npair * one / tp / 1e6, 3), "hbm_floor_us": round(nf * one / HBM_BYTES_PER_US, 2),
                          "pair_over_fused": round(tp / tf, 3)}), flush=True)


def block_dropout_leg(B, N, D, heads, dtype, args):
    """a ConformerBlock's train step (forward + backward) with the forks' rates against the same block with every rate zero"""
    from htrvt_amd import conformer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    on = conformer.ConformerBlock(D, heads, N, ff_dropout=0.1, attn_dropout=0.1, conv_dropout=0.1, drop_path=0.1,
                                  compute_dtype=dtype).to(dev).train()
    off = conformer.ConformerBlock(D, heads, N, ff_dropout=0.0, attn_dropout=0.0, conv_dropout=0.0, drop_path=0.0,
                                   compute_dtype=dtype).to(dev).train()
    x = torch.randn(B, N, D, device=dev)
    dy = torch.randn(B, N, D, device=dev)

    def step(m):
        def fn():
            xr = x.clone().requires_grad_(True)
            m(xr).backward(dy)
            m.zero_grad(set_to_none=True)
        return fn
    (t1, l1, h1), (t0, l0, h0) = alternated_us([step(on), step(off)], max(1, args.reps // 4), args.samples)
    print(json.dumps({"leg": "block_train_dropout", "B": B, "N": N, "D": D, "dtype": str(dtype).split(".")[1],
                      "rates": "ff 0.1 attn 0.1 conv 0.1 path 0.1", "us": round(t1, 1), "us_min": round(l1, 1), "us_max": round(h1, 1),
                      "zero_rates_us": round(t0, 1), "zero_min": round(l0, 1), "zero_max": round(h0, 1),
                      "over_zero_rates": round(t1 / t0, 3)}), flush=True)


LEGS = ("mixer", "se", "dropnorm", "block_dropout")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of " + ", ".join(LEGS))
    args = ap.parse_args()
    legs = args.legs.split(",")
    for dtype in (torch.bfloat16, torch.float32):
        if "mixer" in legs:
            for N in (128, 64, 256):
                mixer_legs(args.batch, N, 384, 3, dtype, args)
        if "se" in legs:
            se_legs(args.batch, 128, 768, dtype, args)
        if "dropnorm" in legs:
            for p, p_path in ((0.1, 0.1), (0.0, 0.1)):         # the forks' rates; drop-path alone (no per-element hash)
                dropnorm_legs(args.batch * 128, 768, 128, dtype, p, p_path, args)
        if "block_dropout" in legs:
            block_dropout_leg(args.batch, 128, 768, 6, dtype, args)


if __name__ == "__main__":
    main()
