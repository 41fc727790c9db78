#!/usr/bin/env python3
"""Times of the validation post-processing on one MI355X (device events after warm-up), one JSON line per leg, all from
one process:
  post      htrvt_ctc_greedy_decode + htrvt_error_counts per batch (and each alone) at T = 256, C = 80 with bench.py's
            synthetic targets (lengths 20 .. 90), for three kinds of logits: `labels` = the targets rendered into frames
            with one symbol in ten substituted (what a trained model emits: about as many decoded symbols as the label
            has), `model` = the untrained model's own logits (long repeats: a dozen decoded symbols) and `random` = normal
            noise (nearly every frame a new symbol: about 250 decoded symbols, the longest tables T = 256 allows).
            decode_us / counts_us / post_us are per call through the Python surface, as a validation loop issues them
            (device time or host issue time, whichever is longer); kernel_us = [decode, counts] are the two C entry points
            alone on preallocated buffers, i.e. the device time of each kernel
  forward   the eval forward + fused CTC loss (want_grad=False) of create_model(80, [64, 1024]) in bfloat16 at the same
            batch, alternated with the post-processing, and the share post / forward
  host      the reference's host path restated: log-softmax, device-to-host copy of the [T,B,C] log-probs, a
            converter.decode-style loop over the frames and a Python Levenshtein table over characters and words, wall
            clock, once.  An UPPER bound of the reference's cost: it runs the C `editdistance`, which is not installed.
    python tools/bench_valid.py [--iters 50] [--batches 128,8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def rendered_logits(targets, lengths, T, C, seed):
    """frames whose arg-max spells each label with one symbol in ten substituted, blanks between repeats and after"""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((len(lengths), T, C)).astype(np.float32)
    o = 0
    for b, n in enumerate(lengths.tolist()):
        t, last = 0, 0
        for c in targets[o:o + n].tolist():
            if rng.random() < 0.1:
                c = int(rng.integers(1, C))
            if c == last and t < T:
                x[b, t, 0] += 9.0
                t += 1
            for _ in range(int(rng.integers(1, 3))):
                if t < T:
                    x[b, t, c] += 9.0
                    t += 1
            last = c
        x[b, t:, 0] += 9.0
        o += n
    return x


def host_path(logits, converter, labels):
    """valid.py:34-75 with the logits already computed, on the host; returns (seconds, CER, WER)"""
    import numpy as np
    import valid_cases as VC
    t0 = time.perf_counter()
    lp = logits.permute(1, 0, 2).log_softmax(2).cpu().numpy()          # [T,B,C] to the host
    idx = lp.argmax(2).transpose(1, 0)
    preds = []
    for row in idx.tolist():
        s = []
        for i, c in enumerate(row):
            if c != 0 and not (i > 0 and row[i - 1] == c) and c < len(converter.character):
                s.append(converter.character[c])
        preds.append("".join(s))
    _, cer, wer = VC.metric_loop(preds, labels)
    return time.perf_counter() - t0, cer, wer, float(np.mean([len(p) for p in preds]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", default="128,8")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_valid.py measures on an MI355X: no GPU found")
    import bench
    import valid_cases as VC
    import htrvt_amd
    from htrvt_amd import valid
    from htrvt_amd.ctc import ctc_forward_backward, greedy_decode, stage_targets
    from htrvt_amd._lib import check, lib
    from htrvt_amd.model import HTR_VT
    from htrvt_amd.ops import ptr, stream

    T, C = 256, 80
    # 79 characters with a space and some punctuation among them: words of a few characters, as in a text line
    alphabet = list(" .,'-" + "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789" + "!?;:()\"&/*+=")[:C - 1]
    conv = VC.Converter(alphabet)
    torch.manual_seed(0)
    model = HTR_VT.create_model(nb_cls=C, img_size=[64, 1024], compute_dtype=torch.bfloat16).cuda().eval()
    for B in [int(v) for v in a.batches.split(",")]:
        x, tg, tl = bench.synthetic_batch(B, 64, 1024, C, T, seed=0)
        x = x.cuda()
        staged = stage_targets(tg, tl, "cuda")
        labels, o = [], 0
        for n in tl.tolist():
            labels.append("".join(conv.character[c] for c in tg[o:o + n].tolist()))
            o += n
        with torch.no_grad():
            y_model = model(x).float().contiguous()
        assert tuple(y_model.shape) == (B, T, C)
        inputs = {"labels": torch.from_numpy(rendered_logits(tg, tl, T, C, 1)).cuda(), "model": y_model,
                  "random": torch.randn(B, T, C, generator=torch.Generator().manual_seed(2)).cuda()}

        def forward():
            with torch.no_grad():
                ctc_forward_backward(model(x).float(), None, None, want_grad=False, staged=staged)

        res = {"forward": []}
        decoded = {k: greedy_decode(v, ncharacter=len(conv.character)) for k, v in inputs.items()}
        legs = {"forward": forward}
        for k, v in inputs.items():
            legs[k + ".decode"] = lambda v=v: greedy_decode(v, ncharacter=len(conv.character))
            legs[k + ".counts"] = lambda k=k: valid.error_counts(decoded[k], None, None, conv, staged=staged)
            legs[k + ".post"] = lambda v=v: valid.error_counts(v, None, None, conv, staged=staged)
        canon, kind = valid.symbol_tables(conv, "cuda")
        counts = torch.empty(B, 4, dtype=torch.int32, device="cuda")
        for k, v in inputs.items():
            idx, lens = decoded[k]
            legs[k + ".k_decode"] = lambda v=v, idx=idx, lens=lens: check(lib.htrvt_ctc_greedy_decode(
                ptr(v), B, T, C, C, len(conv.character), ptr(idx), ptr(lens), stream()))
            legs[k + ".k_counts"] = lambda idx=idx, lens=lens: check(lib.htrvt_error_counts(
                ptr(idx), T, ptr(lens), ptr(staged[0]), ptr(staged[1]), ptr(staged[2]), ptr(canon), ptr(kind), canon.numel(), B, T,
                staged[3], ptr(counts), None, stream()))
        for _ in range(2):                                  # alternated: a drift of the box shows in both columns
            for name, fn in legs.items():
                res.setdefault(name, []).append(round(timed(fn, a.iters), 1))
        fwd = min(res["forward"])
        for k in inputs:
            emit(leg="post", B=B, T=T, C=C, logits=k, mean_decoded=round(float(decoded[k][1].float().mean()), 1),
                 decode_us=res[k + ".decode"], counts_us=res[k + ".counts"], post_us=res[k + ".post"],
                 kernel_us=[min(res[k + ".k_decode"]), min(res[k + ".k_counts"])],
                 share_of_forward=round(min(res[k + ".post"]) / fwd, 4))
        emit(leg="forward", B=B, T=T, C=C, dtype="bf16", forward_ctc_us=res["forward"])
        for k, v in inputs.items():
            sec, cer, wer, mean_len = host_path(v, conv, labels)
            counts = valid.error_counts(v, None, None, conv, staged=staged).sum(0).tolist()
            assert (cer, wer) == (counts[0] / float(counts[1]), counts[2] / float(counts[3])), "host and device metrics differ"
            emit(leg="host", B=B, logits=k, host_ms=round(sec * 1000.0, 1), mean_decoded=round(mean_len, 1), CER=round(cer, 4),
                 WER=round(wer, 4), note="upper bound of the reference: Python Levenshtein in place of the C editdistance")


if __name__ == "__main__":
    main()
