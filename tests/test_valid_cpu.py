"""The host side of htrvt_amd.valid against the reference's recorded validation run (tests/golden/valid.npz, written by
tools/make_goldens_valid.py): the restated word split, metric loop and symbol tables reproduce every word list, distance
and return value the reference formed.  No GPU."""
import numpy as np
import pytest

import valid_cases as VC


@pytest.fixture(scope="module")
def golden(golden_dir):
    return VC.load_golden(golden_dir)


def test_word_split_reproduces_every_recorded_word_list(golden):
    for s, want in golden["probes"]:
        assert VC.wer_words(s) == want, repr(s)
    for name in ("a87", "dup"):
        g = golden[name]
        for p, lab, (pw, gw) in zip(g.preds_str, g.all_labels, g.words):
            assert VC.wer_words(p) == pw and VC.wer_words(lab) == gw, (p, lab)


def test_metric_loop_reproduces_the_recorded_distances_and_rates(golden):
    for name in ("a87", "dup"):
        g = golden[name]
        rows, cer, wer = VC.metric_loop(g.preds_str, g.all_labels)
        assert rows == g.rows()
        assert cer == g.CER and wer == g.WER
        conv = VC.Converter(g.alphabet)
        decoded = [s for batch in g.logits for s in VC.greedy_strings(batch, conv)]
        assert decoded == g.preds_str


def test_all_empty_labels_divide_by_zero():
    with pytest.raises(ZeroDivisionError):
        VC.metric_loop(["a", ""], ["", ""])


def test_kind_agrees_with_the_recorded_word_lists_for_every_alphabet_character(golden):
    from htrvt_amd import valid as V
    words = dict(golden["probes"])
    g = golden["a87"]
    conv = VC.Converter(g.alphabet)
    canon, kind = V.symbol_tables_host(conv)
    assert len(canon) == len(kind) == 90 and kind[0] == V.ORDINARY
    for i in range(1, 90):
        c = conv.character[i] if i < len(conv.character) else {v: k for k, v in conv.dict.items()}[i]
        inside, alone = words["x" + c + "y"], words[c]
        if kind[i] == V.SEPARATOR:
            assert inside == ["x", "y"] and alone == [""], repr(c)
        elif kind[i] == V.PUNCT:
            assert inside == ["x", c, "y"] and alone == [c], repr(c)
        elif kind[i] == V.EDGE_SPACE:
            assert inside == ["x" + c + "y"] and alone == [""], repr(c)
        else:
            assert kind[i] == V.ORDINARY and inside == ["x" + c + "y"] and alone == [c], repr(c)
    assert kind[conv.dict["\\"]] == V.ORDINARY and kind[conv.dict["\t"]] == V.EDGE_SPACE
    assert sorted(c for c in g.alphabet if kind[conv.character.index(c)] == V.PUNCT) == sorted(VC.PUNCT)


def test_symbol_tables_identify_characters_not_indices(golden):
    from htrvt_amd import valid as V
    a87 = VC.Converter(golden["a87"].alphabet)
    canon, kind = V.symbol_tables_host(a87)
    for c, far in (("[", 88), ("]", 89)):
        near = a87.character.index(c)
        assert a87.dict[c] == far and near < 88 and canon[far] == canon[near] == near and kind[far] == kind[near] == V.PUNCT
    assert sorted(set(canon.tolist())) == list(range(88))          # everything else is its own class
    dup = VC.Converter(golden["dup"].alphabet)
    canon, kind = V.symbol_tables_host(dup)
    assert len(canon) == len(dup.character)
    for i, c in enumerate(dup.character):
        assert canon[i] == dup.character.index(c)                  # the first index of the character
        assert canon[dup.dict[c]] == canon[i] if i else canon[0] == 0


def test_index_counts_over_the_tables_reproduce_the_recorded_counts(golden):
    """the reference counts through class indices: predictions by the index the decode emits (the first of a duplicated
    character), labels by converter.dict (the last, or 88 / 89)"""
    from htrvt_amd import valid as V
    for name in ("a87", "dup"):
        g = golden[name]
        conv = VC.Converter(g.alphabet)
        canon, kind = V.symbol_tables_host(conv)
        for p, lab, want in zip(g.preds_str, g.all_labels, g.rows()):
            pi = [conv.character.index(c) for c in p]
            ti = [conv.dict[c] for c in lab]
            assert VC.index_counts(pi, ti, canon, kind) == want, (p, lab)


def test_index_counts_on_the_word_cases_agree_with_the_string_metric():
    from htrvt_amd import valid as V
    conv = VC.word_converter()
    canon, kind = V.symbol_tables_host(conv)
    for p, t in VC.word_cases():
        want = [VC.levenshtein(p, t), len(t), VC.levenshtein(VC.wer_words(p), VC.wer_words(t)), len(VC.wer_words(t))]
        got = VC.index_counts(*(conv.encode_host([s])[0] for s in (p, t)), canon, kind)
        assert got == want, (p, t)
    assert np.array_equal(canon, np.arange(len(canon)))
