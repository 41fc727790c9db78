#!/usr/bin/env python3
"""The SGM head's cost on one MI355X, one JSON line per leg (B = 128, 64 x W = 1024 lines, line lengths drawn as bench.py
draws them: 20 .. 89 characters):
  context  make_context_batch: the drop-in (one host pass, one pinned upload, one kernel) vs an eager restatement of the
           forks' per-character loop
  head     SGMHead forward + backward, bfloat16 and float32: the drop-in vs an eager torch restatement on the same GPU
  step     model forward + backward + CTC with the feature tap and the head, vs the plain step (bfloat16): the SGM overhead
    python tools/bench_sgm.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import htrvt_amd  # noqa: E402,F401
import sgm_cases as C  # noqa: E402
from htrvt_amd.sgm.model import HTR_VT  # noqa: E402
from htrvt_amd.sgm.model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch  # noqa: E402


def texts_of(B, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 90, size=B)
    return ["".join(C.ALPHABET[i] for i in rng.integers(0, 79, size=n)) for n in lens]


def eager_context(texts, stoi, S, dev):
    """the forks' loop, restated: small device tensors per character"""
    ids = [torch.tensor([stoi[c] for c in t], dtype=torch.long).to(dev) for t in texts]
    B, Lmax = len(ids), max(t.numel() for t in ids)
    pad, bos, eos = stoi["<pad>"], stoi["<bos_left>"], stoi["<eos>"]
    left = torch.full((B, Lmax, S), pad, dtype=torch.long, device=dev)
    right, tgt = left.clone(), torch.full((B, Lmax), pad, dtype=torch.long, device=dev)
    mask = torch.zeros(B, Lmax, device=dev)
    for b, seq in enumerate(ids):
        L = seq.numel()
        tgt[b, :L] = seq
        mask[b, :L] = 1
        for i in range(L):
            lc = seq[max(0, i - S):i]
            if lc.numel() < S:
                lc = torch.cat([torch.full((S - lc.numel(),), bos, dtype=torch.long, device=dev), lc])
            left[b, i] = lc
            rc = seq[i + 1:min(L, i + 1 + S)]
            if rc.numel() < S:
                rc = torch.cat([rc, torch.full((S - rc.numel(),), eos, dtype=torch.long, device=dev)])
            right[b, i] = rc
    return left, right, tgt, mask


def eager_head(h, vis, left, right, tgt, mask, dtype):
    """the forks' head as eager torch ops (autocast for bfloat16)"""
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        K = h.kv_norm(vis)

        def q(ids, d):
            return h.q_norm(h.txt_proj(h.emb(ids).mean(2) + d))

        outs = []
        for Q in (q(left, h.dir_left), q(right, h.dir_right)):
            A = torch.einsum('bld,bnd->bln', Q, K) / K.shape[-1] ** 0.5
            outs.append(h.classifier(torch.einsum('bln,bnd->bld', A.softmax(-1), K)))
    V = h.vocab_size
    ll = [F.cross_entropy(o.float().reshape(-1, V), tgt.reshape(-1), reduction='none').view_as(tgt) for o in outs]
    return ((ll[0] + ll[1]) * mask).sum() / (2 * mask.sum().clamp(min=1))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args()
    B, dev = args.batch, torch.device("cuda")
    stoi = build_sgm_vocab(C.Converter())[0]
    texts = texts_of(B)
    ctx = make_context_batch(texts, stoi, 5)
    eager = eager_context(texts, stoi, 5, dev)
    assert all(torch.equal(a, b) for a, b in zip(ctx, eager))
    t_dev = timed(lambda: make_context_batch(texts, stoi, 5), args.reps)
    t_eager = timed(lambda: eager_context(texts, stoi, 5, dev), 2, warm=1)
    print(json.dumps({"leg": "context", "B": B, "Lmax": int(ctx[0].shape[1]), "dropin_ms": round(t_dev, 4),
                      "eager_ms": round(t_eager, 2)}), flush=True)

    N, D = 256, 768
    vis = torch.randn(B, N, D, device=dev)
    for dtype in (torch.bfloat16, torch.float32):
        torch.manual_seed(0)
        h = SGMHead(D, len(stoi), compute_dtype=dtype).cuda().train()
        v = vis.clone().requires_grad_(True)

        def dropin():
            h(v, *ctx)["loss_sgm"].backward()

        def ref():
            eager_head(h, v, *ctx, dtype).backward()
        h.eval()
        print(json.dumps({"leg": "head", "dtype": str(dtype).split(".")[-1], "B": B, "L": int(ctx[0].shape[1]),
                          "dropin_fwd_bwd_ms": round(timed(dropin, args.reps), 3),
                          "eager_fwd_bwd_ms": round(timed(ref, args.reps), 3)}), flush=True)

    from oracle import htrvt_oracle as O
    m = HTR_VT.create_model(80, (64, 1024), compute_dtype=torch.bfloat16).cuda().train()
    x, tg, tl = O.synthetic_batch(B, 64, 1024, 80, m.num_patches, seed=0)
    x = x.cuda()
    tg, tl = torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda()
    head = SGMHead(768, len(stoi), compute_dtype=torch.bfloat16).cuda().train()
    crit = torch.nn.CTCLoss(reduction="none", zero_infinity=True)

    def ctc_of(y):
        lp = y.permute(1, 0, 2).log_softmax(2)
        return crit(lp, tg, torch.full((B,), y.shape[1], dtype=torch.int32, device=dev), tl).mean()

    def plain():
        ctc_of(m(x, 0.4, 8, use_masking=True)).backward()

    def sgm():
        y, f = m(x, 0.4, 8, use_masking=True, return_features=True)
        c = make_context_batch(texts, stoi, 5)
        (ctc_of(y) + head(f, *c)["loss_sgm"]).backward()
    tp, ts = timed(plain, args.reps), timed(sgm, args.reps)
    print(json.dumps({"leg": "step", "B": B, "W": 1024, "plain_ms": round(tp, 3), "sgm_ms": round(ts, 3),
                      "overhead_ms": round(ts - tp, 3)}), flush=True)


if __name__ == "__main__":
    main()
