#!/usr/bin/env python3
"""Generate tests/golden/valid.npz by running the REFERENCE's own validation loop (model_v1/valid.py:9-77 with
utils.CTCLabelConverter and utils.format_string_for_wer) on the CPU.  Dev container only (needs /root/reference); the
fixture is data.

The reference imports `editdistance`, which is not installed: a module of that name is put into sys.modules (as
tools/make_goldens.py does for timm) whose eval() is the textbook Levenshtein table and which records every call, so the
fixture also holds the per-sample distances and the word lists the reference formed.  The loader is a list of
(image, labels) whose image answers .size(0) and .cuda(); the "model" returns stored logits.

Logits are rendered from perturbed labels (characters and words inserted, dropped, substituted; a prediction symbol is
emitted through the FIRST class index of its character, the label through converter.dict, i.e. the last) over quantised
noise, with blank-dominated trailing frames.

    python tools/make_goldens_valid.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/model_v1"
OUT = os.path.join(ROOT, "tests", "golden")

PUNCT = "[]{}/()\"'&+*=<>?.;:,!-—_€#%°"
# 87 distinct characters with '[' and ']' among them: the converter re-maps the brackets to 88 and 89
ALPHA87 = list(PUNCT + " \n\t\\" + "abcdefghijklmnopqrstuvwxyz" + "ABCDEFGHIJKLMNOPQRSTUVWXYZ" + "012")
assert len(ALPHA87) == len(set(ALPHA87)) == 87
LABELS87 = [
    ["it's  a-b.", " [ab] {cd} ", "a/b (c) \"d\" &+*=", "<e>?f;g:h,i!", "j—k_l€m#n%o°", ""],
    ["   ", "ab\ncd\tef", "a\\b c", "\tab cd\t", "the cat sat on the mat", "]x[ y"],
]
# 'a' and 'e' occur twice: converter.dict keeps the later index, converter.character both
ALPHADUP = list("abcdea ef.")
LABELSDUP = [
    ["a bad cafe.", "dead beef", "", "abc abc.", "face  fed", " e a "],
    ["cab. bead", "a", "fade.a", "deaf ace", "bee", "ebb a.e"],
]


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def install_editdistance(calls):
    mod = types.ModuleType("editdistance")

    def _eval(a, b):
        d = levenshtein(a, b)
        calls.append((a, b, d))
        return d

    mod.eval = _eval
    sys.modules["editdistance"] = mod


class FakeImage:
    def __init__(self, n):
        self.n = n

    def size(self, dim):
        assert dim == 0
        return self.n

    def cuda(self):
        return self


def perturb(label, alphabet, rng):
    words = label.split(" ")
    if len(words) > 2 and rng.random() < 0.4:
        words.pop(int(rng.integers(len(words))))
    if len(words) > 1 and rng.random() < 0.3:
        k = int(rng.integers(len(words)))
        words.insert(k, words[k])
    out = []
    for ch in " ".join(words):
        r = rng.random()
        if r < 0.08:
            continue
        if r < 0.16:
            out.append(alphabet[int(rng.integers(len(alphabet)))])
            continue
        out.append(ch)
        if r > 0.93:
            out.append(alphabet[int(rng.integers(len(alphabet)))])
    if not label and rng.random() < 0.5:
        out = [alphabet[int(rng.integers(len(alphabet)))] for _ in range(3)]
    return "".join(out)


def render(pred, character, T, C, extra, rng):
    """frames whose arg-max decodes to `pred` (cut where T runs out); `extra`: class indices beyond len(character) that the
    decode has to drop, sprinkled in"""
    x = rng.integers(-8, 9, size=(T, C)).astype(np.float32) / 8.0
    t, last = 0, 0
    frames = []
    for ch in pred:
        c = character.index(ch)
        if c == last:
            frames.append(0)
        frames.extend([c] * int(rng.integers(1, 3)))
        last = c
        if extra and rng.random() < 0.15:
            frames.append(int(extra[int(rng.integers(len(extra)))]))
            last = frames[-1]
    frames = frames[:T - 4]
    for t in range(T):
        x[t, frames[t] if t < len(frames) else 0] += 8.0
    return x


def run_group(name, alphabet, label_batches, T, seed, out, calls):
    from utils import utils as ref_utils
    import valid as ref_valid
    conv = ref_utils.CTCLabelConverter(alphabet)
    C = max(len(conv.character), max(conv.dict.values()) + 1)
    extra = [i for i in range(len(conv.character), C)]
    rng = np.random.default_rng(seed)
    logits = np.stack([np.stack([render(perturb(s, alphabet, rng), conv.character, T, C, extra, rng) for s in labels])
                       for labels in label_batches])
    del calls[:]
    it = iter(range(len(label_batches)))
    model = lambda image: torch.from_numpy(logits[next(it)])      # noqa: E731
    loader = [(FakeImage(len(labels)), list(labels)) for labels in label_batches]
    crit = torch.nn.CTCLoss(reduction="none", zero_infinity=True)
    val_loss, cer, wer, preds_str, all_labels = ref_valid.validation(model, crit, loader, conv)
    chars = [c for c in calls if isinstance(c[0], str)]
    words = [c for c in calls if not isinstance(c[0], str)]
    assert len(chars) == len(words) == len(all_labels) and [c[1] for c in chars] == all_labels
    out[f"{name}.alphabet"] = np.array(alphabet)
    out[f"{name}.logits"] = logits
    out[f"{name}.labels"] = np.array(label_batches)
    out[f"{name}.val_loss"] = np.float64(val_loss)
    out[f"{name}.CER"] = np.float64(cer)
    out[f"{name}.WER"] = np.float64(wer)
    out[f"{name}.preds_str"] = np.array(preds_str)
    out[f"{name}.ed_char"] = np.array([c[2] for c in chars], np.int32)
    out[f"{name}.ed_word"] = np.array([c[2] for c in words], np.int32)
    out[f"{name}.words"] = np.array(json.dumps([[c[0], c[1]] for c in words]))
    assert list(out[f"{name}.preds_str"]) == preds_str and [list(b) for b in out[f"{name}.labels"]] == label_batches
    print(name, "val_loss", val_loss, "CER", cer, "WER", wer)
    for p, g, c, w in zip(preds_str, all_labels, chars, words):
        print("   ", repr(g), "->", repr(p), c[2], w[2], w[0], w[1])


def main():
    sys.path.insert(0, REF)
    torch.set_num_threads(4)
    out, calls = {}, []
    install_editdistance(calls)
    run_group("a87", ALPHA87, LABELS87, 64, 11, out, calls)
    run_group("dup", ALPHADUP, LABELSDUP, 48, 12, out, calls)
    # the formatting rule itself on every single character of the 87-alphabet and a few strings around the edges
    from utils import utils as ref_utils
    probes = ["x" + c + "y" for c in ALPHA87] + [c for c in ALPHA87] + [
        "it's  a-b.", "a\\b", "", " ", "\n", "\t", " \t a \t ", "a\tb", "\ta", "a\t", "a \n b", "--", "a--b", " . ", "\x0ba\x0c"]
    out["format.probes"] = np.array(json.dumps(probes))
    out["format.words"] = np.array(json.dumps([ref_utils.format_string_for_wer(s).split(" ") for s in probes]))
    np.savez_compressed(os.path.join(OUT, "valid.npz"), **out)
    print("bytes", os.path.getsize(os.path.join(OUT, "valid.npz")))


if __name__ == "__main__":
    main()
