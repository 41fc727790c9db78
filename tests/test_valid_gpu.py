"""htrvt_error_counts (csrc/valid.hip) and the valid.py drop-in on the GPU: exact integers against the textbook Levenshtein
table in Python (tests/valid_cases.py) and against the reference's recorded validation run (tests/golden/valid.npz).
Every refusal is decided on the host before a launch; nothing here provokes a fault."""
import numpy as np
import pytest
import torch

import valid_cases as VC

pytestmark = pytest.mark.gpu


def _env():
    import htrvt_amd  # noqa: F401
    from htrvt_amd import ops, valid
    from htrvt_amd._lib import lib
    return ops, lib, valid


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _pack(pairs, pad=0, fill=7):
    """pred [B][max_pred + pad] (the tail of every row holds `fill`, which must not be read), ragged flat targets"""
    B = len(pairs)
    max_pred = max([len(p) for p, _ in pairs] + [1])
    pred = np.full((B, max_pred + pad), fill, np.int32)
    for b, (p, _) in enumerate(pairs):
        pred[b, :len(p)] = p
    tl = np.array([len(t) for _, t in pairs], np.int32)
    off = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int32)
    flat = np.array([v for _, t in pairs for v in t] + [fill], np.int32)
    return pred, np.array([len(p) for p, _ in pairs], np.int32), flat, tl, off, max_pred, int(tl.max())


def _run(pairs, canon, kind, pad=0, totals=None, max_tgt=None):
    ops, lib, _ = _env()
    pred, pl, flat, tl, off, max_pred, mt = _pack(pairs, pad)
    d = [_dev(pred, np.int32), _dev(pl, np.int32), _dev(flat, np.int32), _dev(tl, np.int32), _dev(off, np.int32),
         _dev(canon, np.int32), _dev(kind, np.uint8)]
    counts = torch.full((len(pairs), 4), -1, dtype=torch.int32, device="cuda")
    rc = lib.htrvt_error_counts(d[0].data_ptr(), pred.shape[1], d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                d[5].data_ptr(), d[6].data_ptr(), len(canon), len(pairs), max_pred, mt if max_tgt is None else max_tgt,
                                counts.data_ptr(), None if totals is None else totals.data_ptr(), ops.stream())
    assert rc == 0, lib.htrvt_last_error().decode()
    torch.cuda.synchronize()
    return counts.cpu().tolist()


def _want(pairs, canon, kind):
    return [VC.index_counts(p, t, canon, kind) for p, t in pairs]


@pytest.fixture(scope="module")
def pairings():
    """all 100 pairings of the lengths over 11 symbols (one separator, one punctuation) with their Python counts"""
    canon, kind = VC.plain_tables(12)
    pairs = VC.random_pairs(np.random.default_rng(5), 12)
    return pairs, canon, kind, _want(pairs, canon, kind)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return VC.load_golden(golden_dir)


def test_every_length_pairing_in_one_launch(pairings):
    pairs, canon, kind, want = pairings
    assert _run(pairs, canon, kind) == want


def test_row_stride_larger_than_max_pred(pairings):
    pairs, canon, kind, want = pairings
    assert _run(pairs[::7], canon, kind, pad=5) == want[::7]


def test_batches_of_one_and_seven_with_ragged_offsets(pairings):
    pairs, canon, kind, want = pairings
    assert _run(pairs[37:38], canon, kind) == want[37:38]
    pick = [3, 99, 40, 0, 58, 91, 15]
    assert _run([pairs[i] for i in pick], canon, kind) == [want[i] for i in pick]


def test_two_symbol_alphabet_identical_and_disjoint_sequences():
    rng = np.random.default_rng(6)
    canon, kind = np.arange(40, dtype=np.int32), np.zeros(40, np.uint8)
    kind[3] = 1
    pairs = VC.random_pairs(rng, 3, [1, 2, 64, 65, 129, 300])          # symbols 1 and 2 only: ties everywhere
    same = rng.integers(1, 20, 200).tolist()
    pairs += [(same, same), (same[:65], same[:65]), (same, [v + 20 for v in same]), ([5] * 130, [6] * 64), ([5] * 64, [5] * 130)]
    assert _run(pairs, canon, kind) == _want(pairs, canon, kind)


def test_longest_target_one_launch_accepts():
    _, lib, _ = _env()
    mt = lib.htrvt_error_counts_max_tgt()
    assert mt >= 512
    rng = np.random.default_rng(7)
    canon, kind = VC.plain_tables(9)
    t = rng.integers(1, 9, mt).tolist()
    p = t[:100] + rng.integers(1, 9, 50).tolist() + t[130:400] + t[420:]   # an edited copy, longer rows than columns in parts
    pairs = [(p, t), (t[:40], t)]
    assert _run(pairs, canon, kind) == _want(pairs, canon, kind)


def test_predictions_up_to_the_decode_limit():
    """beyond 64 KB of LDS per workgroup the launch asks for the large allocation: 8000 and 16384 decoded symbols"""
    rng = np.random.default_rng(8)
    canon, kind = VC.plain_tables(6)
    t = rng.integers(1, 6, 60).tolist()
    pairs = [(rng.integers(1, 6, 8000).tolist(), t), (rng.integers(1, 6, 16384).tolist(), t[:20]), (t, t)]
    assert _run(pairs, canon, kind) == _want(pairs, canon, kind)


def _string_counts(valid, conv, cases):
    pairs = [tuple(conv.encode_host([s])[0] for s in c) for c in cases]
    pred, pl, flat, tl, _, _, _ = _pack(pairs)
    got = valid.error_counts((_dev(pred, np.int32), _dev(pl, np.int32)), flat[:-1], tl, conv)
    return got.cpu().tolist()


def test_word_level_cases():
    """words that differ in the last character or only in length, a word of 70 characters, punctuation runs, and the
    one-empty-word rule on either side"""
    _, _, valid = _env()
    conv = VC.word_converter()
    cases = VC.word_cases()
    want = [[VC.levenshtein(p, t), len(t), VC.levenshtein(VC.wer_words(p), VC.wer_words(t)), len(VC.wer_words(t))] for p, t in cases]
    assert want[cases.index(("", "a"))] == [1, 1, 1, 1] and want[cases.index(("", ""))] == [0, 0, 0, 1]
    assert _string_counts(valid, conv, cases) == want


def test_identity_is_by_character(golden):
    """the 87-character alphabet (label '[' = 88, decoded '[' = its own index) and the duplicated characters give the
    reference's recorded counts, from the logits"""
    _, _, valid = _env()
    for name in ("a87", "dup"):
        g = golden[name]
        conv = VC.Converter(g.alphabet)
        got = []
        for logits, labels in zip(g.logits, g.labels):
            text, lens = conv.encode_host(labels)
            got += valid.error_counts(torch.from_numpy(logits).cuda(), text, lens, conv).cpu().tolist()
        assert got == g.rows(), name


def test_out_of_range_indices_stand_for_themselves(pairings):
    pairs, canon, kind, want = pairings
    pick = [12, 45, 78, 23, 66]
    base = [pairs[i] for i in pick]
    odd = list(base)
    odd[1] = ([1000000, -5] + base[1][0][2:], base[1][1])
    odd[3] = (base[3][0], base[3][1][:3] + [99999, -1, 2 ** 31 - 1] + base[3][1][6:])
    got = _run(odd, canon, kind)
    assert got == _want(odd, canon, kind)
    assert [got[i] for i in (0, 2, 4)] == [want[pick[i]] for i in (0, 2, 4)]


def test_totals_accumulate_over_launches_and_may_be_null(pairings):
    pairs, canon, kind, want = pairings
    totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    a, b = slice(0, 30), slice(30, 41)
    assert _run(pairs[a], canon, kind, totals=totals) == want[a]
    assert _run(pairs[b], canon, kind, totals=totals) == want[b]
    assert totals.cpu().tolist() == np.array(want[a] + want[b], np.int64).sum(0).tolist()
    assert _run(pairs[b], canon, kind, totals=None) == want[b]


class _Stub:
    """a model that returns the stored logits of its call, on the device"""

    def __init__(self, batches):
        self.batches, self.calls = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in batches], 0

    def __call__(self, image):
        assert image.is_cuda
        self.calls += 1
        return self.batches[self.calls - 1]


def test_validation_is_the_reference_loop(golden):
    _, _, valid = _env()
    for name in ("a87", "dup"):
        g = golden[name]
        conv = VC.Converter(g.alphabet)
        loader = [(torch.zeros(len(labels), 1, 4, 4), list(labels)) for labels in g.labels]
        val_loss, cer, wer, preds_str, labels = valid.validation(_Stub(g.logits), None, loader, conv)
        assert preds_str == g.preds_str and labels == g.all_labels
        assert cer == g.CER and wer == g.WER and isinstance(cer, float)
        assert abs(val_loss - g.val_loss) <= 1e-5 * abs(g.val_loss), (val_loss, g.val_loss)


def test_validation_with_only_empty_labels_divides_by_zero(golden):
    _, _, valid = _env()
    g = golden["dup"]
    conv = VC.Converter(g.alphabet)
    with pytest.raises(ZeroDivisionError):
        valid.validation(_Stub(g.logits[:1]), None, [(torch.zeros(6, 1, 4, 4), [""] * 6)], conv)


def _sentinel(ops, lib):
    a = torch.ones(256, 64, dtype=torch.bfloat16, device="cuda")
    c = torch.empty(256, 256, dtype=torch.bfloat16, device="cuda")
    ops.gemm(a, a, c, dtype=torch.bfloat16, M=256, N=256, K=64, lda=64, ldb=64, ldc=256)
    torch.cuda.synchronize()
    return lib.htrvt_last_kernel().decode()


@pytest.mark.parametrize("what", ["max_tgt", "max_pred", "null pred", "null counts", "nsym", "ld_pred", "B"])
def test_refusals_name_the_limit_and_launch_nothing(what):
    ops, lib, _ = _env()
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    u8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = i32.data_ptr()
    limit = lib.htrvt_error_counts_max_tgt()
    kw = dict(pred=p, ld=8, counts=p, nsym=4, B=2, max_pred=8, max_tgt=8)
    kw.update({"max_tgt": dict(max_tgt=limit + 1), "max_pred": dict(max_pred=16385, ld=16385), "null pred": dict(pred=None),
               "null counts": dict(counts=None), "nsym": dict(nsym=0), "ld_pred": dict(ld=7), "B": dict(B=0)}[what])
    before = _sentinel(ops, lib)
    rc = lib.htrvt_error_counts(kw["pred"], kw["ld"], p, p, p, p, p, u8.data_ptr(), kw["nsym"], kw["B"], kw["max_pred"],
                                kw["max_tgt"], kw["counts"], None, ops.stream())
    msg = lib.htrvt_last_error().decode()
    assert rc < 0 and "htrvt_error_counts" in msg
    expect = {"max_tgt": str(limit), "max_pred": "16384", "null pred": "null", "null counts": "null", "nsym": "nsym", "ld_pred": "ld_pred",
              "B": "B="}[what]
    assert expect in msg, msg
    assert lib.htrvt_last_kernel().decode() == before, "a kernel was launched"
    torch.cuda.synchronize()


def test_cpu_tensors_are_refused():
    _, _, valid = _env()
    conv = VC.word_converter()
    with pytest.raises(RuntimeError):
        valid.error_counts(torch.zeros(2, 8, len(conv.character)), [1, 2], [1, 1], conv)
    with pytest.raises(RuntimeError):
        valid.error_counts((torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)), [1, 2], [1, 1], conv)
