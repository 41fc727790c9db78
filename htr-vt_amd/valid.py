"""Drop-in for model_v1/valid.py: `validation(model, criterion, evaluation_loader, converter)` with the reference's
signature and 5-tuple, computed on the device.

    from htrvt_amd.valid import validation          # instead of `import valid` + `valid.validation` (test.py, train.py)

Per batch: model(image), the fused CTC loss, the greedy decode and htrvt_error_counts (csrc/valid.hip): the Levenshtein
distances of valid.py:49-71 over characters and over the word lists of format_string_for_wer(...).split(" ").  Logits never
leave the device and the host never loops over frames; what comes back per batch is the [B,T] int32 decode (for the
returned strings), and after the loop four integer totals and the loss sum.  `editdistance` is not needed."""
import weakref

import numpy as np
import torch

from ._lib import check, lib
from .ctc import ctc_forward_backward, greedy_decode, stage_targets
from .ops import ptr, stream

# utils/utils.py:176-179 restated.  The first re.sub puts spaces around each of these (the pattern's `\\(` is an escaped
# parenthesis: backslash is not in the set), the second collapses runs of space / newline, then str.strip() and split(" ").
PUNCTUATION = "[]{}/()\"'&+*=<>?.;:,!-—_€#%°"
SEPARATORS = " \n"
ORDINARY, SEPARATOR, PUNCT, EDGE_SPACE = 0, 1, 2, 3


def char_kind(ch):
    """what one character is to the word split: separator, punctuation (a word of its own), other white space (str.strip
    drops it at the ends of the string, inside it is an ordinary character), or ordinary"""
    if ch in SEPARATORS and len(ch) == 1:
        return SEPARATOR
    if ch in PUNCTUATION and len(ch) == 1:
        return PUNCT
    return EDGE_SPACE if len(ch) == 1 and ch.isspace() else ORDINARY


def symbol_tables_host(converter):
    """(canon int32 [nsym], kind uint8 [nsym]) of a CTCLabelConverter (utils/utils.py:55-63).  Index i denotes
    converter.character[i] when i < len(character), else the key of converter.dict whose value is i (the converter re-maps
    '[' and ']' of an 87-character alphabet to 88 and 89, beyond `character`); an index that denotes nothing stands for
    itself.  canon[i] is the lowest index that denotes the same character, so a duplicated alphabet character and the
    re-mapped brackets compare equal to their other index."""
    character = list(converter.character)
    by_value = {int(v): k for k, v in converter.dict.items()}
    nsym = max([len(character)] + [v + 1 for v in by_value])
    canon, kind, first = np.arange(nsym, dtype=np.int32), np.zeros(nsym, dtype=np.uint8), {}
    for i in range(nsym):
        ch = character[i] if i < len(character) else by_value.get(i)
        if ch is None:
            continue
        canon[i] = first.setdefault(ch, i)
        kind[i] = char_kind(ch)
    return canon, kind


_tables = weakref.WeakKeyDictionary()


def symbol_tables(converter, device):
    """symbol_tables_host on the device, built once per converter and device"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("htrvt_amd.valid needs a device on an MI355X (no CPU fallback)")
    try:
        entry = _tables.setdefault(converter, {})
    except TypeError:           # a converter that cannot be weakly referenced is not cached
        entry = {}
    if device not in entry:
        canon, kind = symbol_tables_host(converter)
        entry[device] = (torch.from_numpy(canon).to(device), torch.from_numpy(kind).to(device))
    return entry[device]


def error_counts(logits_or_decoded, targets, target_lengths, converter, staged=None, totals=None):
    """int32 [B,4] on the device: per sample (character edit distance, len(gt), word edit distance, len(gt_words)).
    logits_or_decoded: logits [B,T,C] (greedy-decoded here) or greedy_decode's (idx [B,T] int32, lens [B] int32).
    targets / target_lengths: converter.encode's flat class indices and lengths, or staged = ctc.stage_targets(...) of them.
    totals: optional int64 [4] on the device, the column sums are added to it."""
    if isinstance(logits_or_decoded, (tuple, list)):
        idx, lens = logits_or_decoded
    else:
        if not logits_or_decoded.is_cuda:
            raise RuntimeError("htrvt_amd.valid.error_counts needs device tensors on an MI355X (no CPU fallback)")
        idx, lens = greedy_decode(logits_or_decoded, ncharacter=len(converter.character))
    if not (idx.is_cuda and lens.is_cuda):
        raise RuntimeError("htrvt_amd.valid.error_counts needs device tensors on an MI355X (no CPU fallback)")
    assert idx.dtype == torch.int32 and lens.dtype == torch.int32 and idx.dim() == 2 and idx.stride(1) == 1
    B, T = idx.shape
    tg, tl, off, maxlen = staged if staged is not None else stage_targets(targets, target_lengths, idx.device)
    canon, kind = symbol_tables(converter, idx.device)
    counts = torch.empty(B, 4, dtype=torch.int32, device=idx.device)
    if totals is not None:
        assert totals.is_cuda and totals.dtype == torch.int64 and totals.numel() == 4 and totals.is_contiguous()
    check(lib.htrvt_error_counts(ptr(idx), idx.stride(0), ptr(lens), ptr(tg), ptr(tl), ptr(off), ptr(canon), ptr(kind),
                                 canon.numel(), B, T, maxlen, ptr(counts), ptr(totals), stream()), "error_counts")
    return counts


def _strings(idx, lens, character):
    rows = idx.tolist()
    return ["".join(character[c] for c in row[:n]) for row, n in zip(rows, lens.tolist())]


def validation(model, criterion, evaluation_loader, converter):
    """model_v1/valid.py:9-77 -> (val_loss, CER, WER, all_preds_str, all_labels).  `criterion` is accepted for the
    signature and not called: the loss is htrvt_ctc_loss, = CTCLoss(reduction='none', zero_infinity=True) on the
    log-softmax with every frame as input length (valid.py:33-37)."""
    del criterion
    totals, loss_sum, count = None, None, 0
    all_preds_str, all_labels = [], []
    pending = None      # (pinned idx, pinned lens, event) of the previous batch: its strings are built while this one runs

    def collect(p):
        p[2].synchronize()
        all_preds_str.extend(_strings(p[0], p[1], converter.character))

    for image_tensors, labels in evaluation_loader:
        image = image_tensors.cuda()
        preds = model(image)
        if not preds.is_cuda:
            raise RuntimeError("htrvt_amd.valid.validation needs a model on an MI355X (no CPU fallback)")
        preds = preds.float()
        dev = preds.device
        if totals is None:
            totals = torch.zeros(4, dtype=torch.int64, device=dev)
            loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        # converter.encode (utils/utils.py:65-70) on host lists: the lengths stay on the host, the indices go up pinned
        text = [converter.dict[ch] for s in labels for ch in s]
        staged = stage_targets(torch.tensor(text, dtype=torch.int32), torch.tensor([len(s) for s in labels], dtype=torch.int32), dev)
        nll, _ = ctc_forward_backward(preds, None, None, want_grad=False, staged=staged)
        loss_sum += nll.mean()
        count += 1
        idx, lens = greedy_decode(preds, ncharacter=len(converter.character))
        error_counts((idx, lens), None, None, converter, staged=staged, totals=totals)
        h_idx = torch.empty(idx.shape, dtype=torch.int32, pin_memory=True)
        h_len = torch.empty(lens.shape, dtype=torch.int32, pin_memory=True)
        h_idx.copy_(idx, non_blocking=True)
        h_len.copy_(lens, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        if pending is not None:
            collect(pending)
        pending = (h_idx, h_len, ev)
        all_labels.extend(labels)
    if pending is not None:
        collect(pending)
    tot_ED, length_of_gt, tot_ED_wer, length_of_gt_wer = (totals.tolist() if totals is not None else (0, 0, 0, 0))
    val_loss = (float(loss_sum) if count else 0.0) / count      # no batch at all: ZeroDivisionError, as the reference
    CER = tot_ED / float(length_of_gt)
    WER = tot_ED_wer / float(length_of_gt_wer)
    return val_loss, CER, WER, all_preds_str, all_labels
