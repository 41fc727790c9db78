"""What the validation metrics are, restated in plain Python for the tests of htrvt_amd.valid and htrvt_error_counts
(tests/test_valid_cpu.py, tests/test_valid_gpu.py): the textbook Levenshtein table, the word split the reference applies
before WER, its metric loop, the label converter's two tables, and the same counts over raw class-index sequences.
tests/golden/valid.npz (tools/make_goldens_valid.py: the reference's own validation loop, recorded) pins all of it."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# the characters that become words of their own; backslash is not one of them
PUNCT = set("[]{}/()\"'&+*=<>?.;:,!-—_€#%°")


def levenshtein(a, b):
    """unit-cost insert / delete / substitute distance of two sequences, full table row by row"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
        prev = cur
    return prev[len(b)]


def wer_words(s):
    """the word list WER is taken over: punctuation set apart, runs of space / newline collapsed, ends stripped, split at
    single spaces -- so an empty or all-separator string is [''], one empty word"""
    spaced = "".join(" " + c + " " if c in PUNCT else c for c in s)
    collapsed = []
    for c in spaced:
        if c in " \n":
            if collapsed and collapsed[-1] == " ":
                continue
            c = " "
        collapsed.append(c)
    return "".join(collapsed).strip().split(" ")


def metric_loop(preds_str, labels):
    """-> (per-sample [ed_char, len(gt), ed_word, len(gt_words)], CER, WER) the way the validation loop forms them"""
    rows = []
    for p, g in zip(preds_str, labels):
        pw, gw = wer_words(p), wer_words(g)
        rows.append([levenshtein(p, g), len(g), levenshtein(pw, gw), len(gw)])
    tot = np.array(rows, dtype=np.int64).reshape(-1, 4).sum(0).tolist()
    return rows, tot[0] / float(tot[1]), tot[2] / float(tot[3])


class Converter:
    """the label converter's two tables: class 0 is the blank, a duplicated alphabet character keeps its LAST index in
    `dict` and both in `character`, and an alphabet of 87 distinct characters gets '[' and ']' at 88 and 89"""

    def __init__(self, alphabet):
        alphabet = list(alphabet)
        self.dict = {}
        for i, c in enumerate(alphabet):
            self.dict[c] = i + 1
        if len(self.dict) == 87:
            self.dict["["], self.dict["]"] = 88, 89
        self.character = ["[blank]"] + alphabet

    def encode_host(self, labels):
        return [self.dict[c] for s in labels for c in s], [len(s) for s in labels]


def greedy_strings(logits, converter):
    """arg-max per frame, blanks / repeats / indices beyond `character` dropped -> strings; logits [B,T,C] numpy"""
    out = []
    for row in np.asarray(logits).argmax(-1):
        s, last = [], -1
        for c in row.tolist():
            if c != 0 and c != last and c < len(converter.character):
                s.append(converter.character[c])
            last = c
        out.append("".join(s))
    return out


def index_counts(pred, tgt, canon, kind):
    """[ed_char, len(tgt), ed_word, len(tgt_words)] of two class-index sequences under (canon, kind) tables: an index
    outside the tables stands for itself and is ordinary; kind 0 ordinary, 1 separator, 2 punctuation, 3 white space that
    only counts inside the string"""
    n = len(canon)

    def canonical(seq):
        return [int(canon[v]) if 0 <= v < n else int(v) for v in seq]

    def words(seq):
        sym = canonical(seq)
        kd = [int(kind[v]) if 0 <= v < n else 0 for v in seq]
        lo, hi = 0, len(sym)
        while lo < hi and kd[lo] in (1, 3):
            lo += 1
        while hi > lo and kd[hi - 1] in (1, 3):
            hi -= 1
        out, cur = [], []
        for v, k in zip(sym[lo:hi], kd[lo:hi]):
            if k in (0, 3):
                cur.append(v)
                continue
            if cur:
                out.append(tuple(cur))
                cur = []
            if k == 2:
                out.append((v,))
        if cur:
            out.append(tuple(cur))
        return out or [()]

    pw, tw = words(pred), words(tgt)
    return [levenshtein(canonical(pred), canonical(tgt)), len(tgt), levenshtein(pw, tw), len(tw)]


class Golden:
    """one alphabet group of tests/golden/valid.npz"""

    def __init__(self, npz, name):
        self.alphabet = [str(c) for c in npz[name + ".alphabet"]]
        self.logits = npz[name + ".logits"]                               # [batches, B, T, C] float32
        self.labels = [[str(s) for s in b] for b in npz[name + ".labels"]]
        self.val_loss, self.CER, self.WER = (float(npz[name + "." + k]) for k in ("val_loss", "CER", "WER"))
        self.preds_str = [str(s) for s in npz[name + ".preds_str"]]
        self.ed_char = npz[name + ".ed_char"].tolist()
        self.ed_word = npz[name + ".ed_word"].tolist()
        self.words = json.loads(str(npz[name + ".words"]))                # per sample [pred words, label words]
        self.all_labels = [s for b in self.labels for s in b]

    def rows(self):
        return [[c, len(g), w, len(ws[1])] for c, g, w, ws in zip(self.ed_char, self.all_labels, self.ed_word, self.words)]


def load_golden(golden_dir=None):
    npz = np.load(os.path.join(golden_dir or os.path.join(HERE, "golden"), "valid.npz"))
    probes = json.loads(str(npz["format.probes"]))
    return {"a87": Golden(npz, "a87"), "dup": Golden(npz, "dup"), "probes": list(zip(probes, json.loads(str(npz["format.words"]))))}


# ---- raw sequences for the kernel -------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 300]


def plain_tables(nsym):
    """identity canon, class 1 a separator, class 2 punctuation, everything else ordinary"""
    kind = np.zeros(nsym, np.uint8)
    kind[1], kind[2] = 1, 2
    return np.arange(nsym, dtype=np.int32), kind


def random_pairs(rng, nsym, lengths=LENGTHS):
    """every pairing of the lengths, symbols uniform in [1, nsym): with nsym = 3 nearly every cell of the table is a tie"""
    return [(rng.integers(1, nsym, lp).tolist(), rng.integers(1, nsym, lt).tolist()) for lp in lengths for lt in lengths]


def word_cases():
    """(pred, tgt) as strings over the alphabet of `word_converter()`"""
    long_a = "abcdefghij" * 7                     # one word of 70 characters
    return [
        ("abcd abce abcf", "abcd abcd abcf"),     # words that differ only in their last character
        ("abc abcd ab", "abcd abc abc"),          # words that are equal up to the shorter length
        (long_a + " x", long_a[:-1] + "k x"),     # a word longer than 64 against a near copy
        (long_a, long_a),
        ("a..,b--c", "a.,,b-c"),                  # punctuation runs
        ("...", ".."),
        ("", "a"), ("a", ""), ("", ""), ("   ", ""), ("", "  \n "), (" \n", "a b"), ("a b", "\n\n"),
        ("  a  b  ", "a b"), ("\ta b\t", "a b"), ("a\tb", "a b"), ("\t", "\t\t"),
        ("the cat sat on the mat", "the mat sat on a cat the"),
    ]


def word_converter():
    return Converter("abcdefghijklmnopqrstuvwxyz .,-\n\t")
