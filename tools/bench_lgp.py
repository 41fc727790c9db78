#!/usr/bin/env python3
"""Times of the LGP fork's kernels and model on one MI355X (device events after warm-up), one JSON line per leg:
  kernel    each csrc/lgp.hip kernel, forward and backward, at B = 128, N = 256, G = 64, D = 768, 6 heads of 128, bfloat16,
            with its algorithmic bytes (computed from the shape below) -> bytes/s and the share of the 6.3 TB/s the
            hardware guide calls achievable, next to htrvt_bn_apply (a streaming pass of this library) on a tensor of the
            window kernel's size, measured in the same process
            (each launch repeats on the same buffers, which mostly fit the 256 MiB last-level cache: rates relative to the
            yardstick under the same conditions, not HBM rates)
  window    htrvt_attn_local_* against htrvt_attn_relpos_* (zero table, window 12) at a padding-free length
            (B = 128, N = 240, hd = 128, bfloat16), alternated
  block     forward + backward of one encoder block, LGP next to model_v1: the difference between two-block and
            one-block models (64 x 1024 images, B = 128), alternated
  step      forward + CTC + backward + AdamW through Trainer.step of the four-block LGP model and of model_v1, alternated
  profile   exactly --iters training steps of ONE model (--model lgp | v1), nothing timed: the command to put behind
            `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --` (tools/prof_summary.py DIR OUT --steps ITERS)
    python tools/bench_lgp.py [--iters 30] [--batch 128] [--legs kernel,window,block,step] [--model lgp]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12


def timed(fn, iters, warm=5):
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def rate(leg, name, us, nbytes, **kw):
    bps = nbytes / (us * 1e-6)
    emit(leg=leg, name=name, us=round(us, 1), mbytes=round(nbytes / 1e6, 1), tb_per_s=round(bps / 1e12, 2),
         share_of_6p3=round(bps / HBM_ACHIEVABLE, 3), **kw)


def leg_kernels(iters, B):
    import torch
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import ptr, stream
    BF, es = 1, 2
    N, G, h, hd, w = 256, 64, 6, 128, 12
    D = h * hd
    M = B * N
    dev = "cuda"
    bf = torch.bfloat16
    qkv = torch.randn(M, 3 * D, device=dev).to(bf)
    bias = torch.randn(3 * D, device=dev)
    out, dout = torch.empty(M, D, device=dev, dtype=bf), torch.randn(M, D, device=dev).to(bf)
    dqkv, dpad = torch.empty_like(qkv), torch.empty(B, 2 * D, device=dev)
    sc = hd ** -0.5
    # the library's own streaming pass on a tensor of the window forward's traffic (read 2 bytes, write 2 bytes per element)
    nel = M * 2 * D
    x, y = torch.randn(nel // D, D, device=dev).to(bf), torch.empty(nel // D, D, device=dev, dtype=bf)
    scl, shf = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    us = timed(lambda: check(lib.htrvt_bn_apply(ptr(x), ptr(scl), ptr(shf), None, None, None, ptr(y), nel // D, D, 0, BF, stream())), iters)
    rate("kernel", "htrvt_bn_apply (streaming yardstick)", us, 2 * nel * es)
    us = timed(lambda: check(lib.htrvt_attn_local_fwd(ptr(qkv), ptr(bias), ptr(out), B, N, h, hd, w, sc, BF, stream())), iters)
    rate("kernel", "htrvt_attn_local_fwd", us, (M * 3 * D + M * D) * es)
    us = timed(lambda: check(lib.htrvt_attn_local_bwd(ptr(qkv), ptr(bias), ptr(dout), ptr(dqkv), ptr(dpad), B, N, h, hd, w, sc, BF,
                                                      stream())), iters)
    rate("kernel", "htrvt_attn_local_bwd", us, (M * 3 * D + M * D + M * 3 * D) * es)
    # pooling + LayerNorm: reads x [M][D] once (bins overlap only when G does not divide N), writes z [B G][D]
    xx, z = torch.randn(M, D, device=dev).to(bf), torch.empty(B * G, D, device=dev, dtype=bf)
    mean, rstd = torch.empty(B * G, device=dev), torch.empty(B * G, device=dev)
    us = timed(lambda: check(lib.htrvt_lgp_pool_norm_fwd(ptr(xx), ptr(z), ptr(mean), ptr(rstd), B, N, G, D, 1e-5, BF, stream())), iters)
    rate("kernel", "htrvt_lgp_pool_norm_fwd", us, (M * D + B * G * D) * es)
    dz, dx, ws = torch.randn(B * G, D, device=dev).to(bf), torch.zeros(M, D, device=dev, dtype=bf), torch.empty(2 * B * G, device=dev)
    us = timed(lambda: check(lib.htrvt_lgp_pool_norm_bwd(ptr(dz), ptr(z), ptr(rstd), ptr(ws), ptr(dx), B, N, G, D, 1, BF, stream())), iters)
    rate("kernel", "htrvt_lgp_pool_norm_bwd (accumulating)", us, (2 * M * D + 4 * B * G * D) * es)
    # up-sampling: reads y [B G][D], writes [M][D] with row stride 2 D; backward reads that gradient and y, writes dy
    yg, alpha = torch.randn(B * G, D, device=dev).to(bf), torch.tensor(0.3, device=dev)
    cat = torch.empty(M, 2 * D, device=dev, dtype=bf)
    us = timed(lambda: check(lib.htrvt_lgp_upsample_fwd(ptr(yg), ptr(alpha), cat.data_ptr() + D * es, 2 * D, B, N, G, D, BF, stream())), iters)
    rate("kernel", "htrvt_lgp_upsample_fwd", us, (B * G * D + M * D) * es)
    dcat = torch.randn(M, 2 * D, device=dev).to(bf)
    dy, da = torch.empty_like(yg), torch.zeros((), device=dev)
    ws = torch.empty(lib.htrvt_lgp_upsample_bwd_workspace_floats(B, G), device=dev)
    us = timed(lambda: check(lib.htrvt_lgp_upsample_bwd(dcat.data_ptr() + D * es, 2 * D, ptr(yg), ptr(alpha), ptr(dy), ptr(da), ptr(ws),
                                                        B, N, G, D, BF, stream())), iters)
    rate("kernel", "htrvt_lgp_upsample_bwd", us, (M * D + 2 * B * G * D) * es)


def leg_window(iters, B):
    import torch
    from htrvt_amd import variants as V
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import ptr, stream
    BF = 1
    N, h, hd, w, P = 240, 6, 128, 12, 256
    D, M = h * hd, B * N
    dev, bf = "cuda", torch.bfloat16
    qkv = torch.randn(M, 3 * D, device=dev).to(bf)
    bias = torch.zeros(3 * D, device=dev)
    out, dout, dqkv = torch.empty(M, D, device=dev, dtype=bf), torch.randn(M, D, device=dev).to(bf), torch.empty_like(qkv)
    dpad = torch.empty(B, 2 * D, device=dev)
    table = torch.zeros(2 * P - 1, h, device=dev)
    lse, delta = torch.empty(B * h, N, device=dev), torch.empty(B * h, N, device=dev)
    sc = hd ** -0.5
    assert V.relpos_supported(N, hd, bf, P, w, 0), lib.htrvt_last_error().decode()
    l_f = lambda: check(lib.htrvt_attn_local_fwd(ptr(qkv), ptr(bias), ptr(out), B, N, h, hd, w, sc, BF, stream()))     # noqa: E731
    l_b = lambda: check(lib.htrvt_attn_local_bwd(ptr(qkv), ptr(bias), ptr(dout), ptr(dqkv), ptr(dpad), B, N, h, hd, w, sc, BF, stream()))  # noqa: E731
    r_f = lambda: check(lib.htrvt_attn_relpos_fwd(ptr(qkv), ptr(table), ptr(out), ptr(lse), B, N, h, hd, sc, P, w, 0, BF, stream()))    # noqa: E731
    r_b = lambda: check(lib.htrvt_attn_relpos_bwd(ptr(qkv), ptr(table), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dqkv), None, None,   # noqa: E731
                                                  B, N, h, hd, sc, P, w, 0, BF, stream()))
    res = {}
    for rep in range(2):
        for name, fn in (("local_fwd", l_f), ("relpos_fwd", r_f), ("local_bwd", l_b), ("relpos_bwd", r_b)):
            res.setdefault(name, []).append(round(timed(fn, iters), 1))
    emit(leg="window", B=B, N=N, hd=hd, window=w, us=res,
         fwd_ratio=round(min(res["local_fwd"]) / min(res["relpos_fwd"]), 3), bwd_ratio=round(min(res["local_bwd"]) / min(res["relpos_bwd"]), 3))


def _models(depth, B):
    import torch
    from functools import partial
    from htrvt_amd.lgp.model import HTR_VT as L
    from htrvt_amd.model import HTR_VT as V1
    kw = dict(img_size=[64, 1024], patch_size=(4, 64), embed_dim=768, depth=depth, num_heads=6, mlp_ratio=4,
              norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), compute_dtype=torch.bfloat16)
    torch.manual_seed(0)
    return {"lgp": L.MaskedAutoencoderViT(80, **kw).cuda().train(), "v1": V1.MaskedAutoencoderViT(80, **kw).cuda().train()}


def _batch(B, N):
    import torch
    g = torch.Generator().manual_seed(1)
    img = torch.rand(B, 1, 64, 1024, generator=g).cuda()
    lengths = torch.randint(20, 60, (B,), generator=g, dtype=torch.int32)
    targets = torch.randint(1, 80, (int(lengths.sum()),), generator=g, dtype=torch.int32)
    keep = torch.ones(N)
    keep[40:48] = 0
    return img, targets, lengths, keep


def _alternate(fns, iters, reps=2):
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(round(timed(fn, iters, warm=3) / 1000.0, 3))     # ms
    return out


def leg_block(iters, B):
    import torch
    from htrvt_amd.trainer import Trainer
    img, tg, ln, keep = _batch(B, 256)
    ms = {}
    for depth in (1, 2):
        tr = {k: Trainer(m) for k, m in _models(depth, B).items()}
        r = _alternate({k: (lambda t=t: t.forward_backward(img, tg, ln, keep_mask=keep)) for k, t in tr.items()}, iters)
        ms[depth] = {k: min(v) for k, v in r.items()}
        del tr
        torch.cuda.empty_cache()
    emit(leg="block", B=B, N=256, fwd_bwd_ms_by_depth=ms, lgp_block_ms=round(ms[2]["lgp"] - ms[1]["lgp"], 3),
         v1_block_ms=round(ms[2]["v1"] - ms[1]["v1"], 3))


def leg_step(iters, B):
    from htrvt_amd.trainer import Trainer
    img, tg, ln, keep = _batch(B, 256)
    tr = {k: Trainer(m) for k, m in _models(4, B).items()}
    r = _alternate({k: (lambda t=t: t.step(img, tg, ln, keep_mask=keep)) for k, t in tr.items()}, iters)
    # MACs per token of one block (SURVEY 8(d) extended): LGP 14 D^2 + 24 D + (4 D^2 + 2 G D) G / N, v1 12 D^2 + 2 N D
    N, G, D = 256, 64, 768
    macs = dict(lgp=14 * N * D * D + 4 * G * D * D + 24 * N * D + 2 * G * G * D, v1=12 * N * D * D + 2 * N * N * D)
    emit(leg="step", B=B, N=N, step_ms=r, lgp_over_v1=round(min(r["lgp"]) / min(r["v1"]), 3),
         block_macs_lgp_over_v1=round(macs["lgp"] / macs["v1"], 3))


def leg_profile(iters, B, model="lgp"):
    import torch
    from htrvt_amd.trainer import Trainer
    img, tg, ln, keep = _batch(B, 256)
    tr = Trainer(_models(4, B)[model])
    for _ in range(iters):
        tr.step(img, tg, ln, keep_mask=keep)
    torch.cuda.synchronize()
    emit(leg="profile", model=model, steps=iters, B=B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--legs", default="kernel,window,block,step")
    ap.add_argument("--model", default="lgp", choices=("lgp", "v1"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_lgp.py measures on an MI355X: no GPU found")
    import htrvt_amd  # noqa: F401
    legs = dict(kernel=leg_kernels, window=leg_window, block=leg_block, step=leg_step,
                profile=lambda it, b: leg_profile(it, b, a.model))
    for name in a.legs.split(","):
        legs[name](a.iters, a.batch)


if __name__ == "__main__":
    main()
