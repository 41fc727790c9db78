"""The multi-mask ("mms") SGM forks' per-sample token-mask generators without device round trips.

Semantics: model_sgm_mms_attach/model/HTR_VT.py:222-346 (identical in model_sgm_mms_detach and the other mms forks built
on that file).  Every function returns what the fork's method returns -- bool [B, L] on `device`, True = masked, or the
float keep mask [B, L, 1] (1 keep / 0 mask token) -- and consumes exactly the fork's random streams, in its order:
    mask_random_1d    torch.rand(B, L, device=device) + argsort (device work, nothing comes back to the host)
    mask_block_1d     Python's random.randint, two draws per trial
    mask_span_1d      Python's random.randint, two draws per trial
    mask_span_old_1d  one torch.randint(..., (1,), device=device) per span
so after random.seed(s); torch.manual_seed(s) the masks and the generator states left behind are the fork's.

The fork keeps the block and span bookkeeping in device tensors and calls .item() in every trial (up to 10 000 per
sample): thousands of host-device synchronisations per training step.  Here those loops run over numpy arrays in host
memory and the finished [B, L] mask is uploaded ONCE, through pinned memory (as Engine._begin_forward uploads a host
mask).  The only synchronisations left are the ones span_old needs to stay stream-exact: its start positions come from
the DEVICE generator, one .item() per span (a handful per call; the fork has them too).

Not covered: the SVTR fork carries its own, simplified block and span generators (model_sgm_mms_svtr .../svtr.py:333-388:
no spacing rule, `covered += s`, ...).  They draw differently and give other masks; this module does not serve them.
"""
import random

import numpy as np
import torch

DEFAULT_RATIOS = {"random": 0.50, "block": 0.25, "span": 0.25}      # HTR_VT.py:336
TRIAL_CAP = 10000                                                    # HTR_VT.py:248,290


def _upload(mask, device):
    """host bool array -> bool tensor on `device`; a device copy goes through pinned memory and does not wait"""
    t = torch.from_numpy(mask)
    device = torch.device(device)
    if device.type == "cpu":
        return t
    return t.pin_memory().to(device, non_blocking=True)


def _zeros(B, L, device):
    return torch.zeros(B, L, dtype=torch.bool, device=device)


def mask_random_1d(B, L, ratio, device):
    """HTR_VT.py:222-233: round(ratio L) tokens per sample, the first of an argsort of uniform noise"""
    if ratio <= 0.0:
        return _zeros(B, L, device)
    num = int(round(ratio * L))
    if num <= 0:
        return _zeros(B, L, device)
    noise = torch.rand(B, L, device=device)
    idx = noise.argsort(dim=1)[:, :num]
    mask = _zeros(B, L, device)
    mask.scatter_(1, idx, True)
    return mask


def _block_host(B, L, ratio, min_block=2):
    """the loops of HTR_VT.py:243-258 over a host array: (mask bool [B, L], trials per sample)"""
    target = int(round(ratio * L))
    mask = np.zeros((B, L), dtype=np.bool_)
    trials = []
    for b in range(B):
        covered, n = 0, 0
        for _ in range(TRIAL_CAP):
            if covered >= target:
                break
            n += 1
            remain = max(1, target - covered)
            blk = random.randint(min_block, max(min_block, min(remain, L)))
            start = random.randint(0, max(0, L - blk))
            seg = mask[b, start:start + blk]
            covered += seg.size - int(seg.sum())
            seg[:] = True
        trials.append(n)
    return mask, trials


def mask_block_1d(B, L, ratio, device, min_block=2):
    """HTR_VT.py:235-259: contiguous blocks of min_block ... remaining-target tokens until round(ratio L) are covered"""
    if ratio <= 0.0:
        return _zeros(B, L, device)
    return _upload(_block_host(B, L, ratio, min_block)[0], device)


def _span_host(B, L, ratio, max_span):
    """the loops of HTR_VT.py:272-304 over a host array: (mask bool [B, L], trials per sample)"""
    L = int(L)
    max_span = int(max(1, min(max_span, L)))
    target = int(round(ratio * L))
    fixed_k = None if ratio <= 0.4 else (1 if ratio <= 0.7 else 0)     # None: spacing = the span's own length
    mask = np.zeros((B, L), dtype=np.bool_)
    trials = []
    for b in range(B):
        used = mask[b]
        covered, n = 0, 0
        for _ in range(TRIAL_CAP):
            if covered >= target:
                break
            n += 1
            s = random.randint(1, max_span)
            if s > L:
                s = L
            l = random.randint(0, L - s)
            r = l + s - 1
            k = s if fixed_k is None else fixed_k
            left_ok = (l - k) < 0 or not used[max(0, l - k):l].any()
            right_ok = (r + 1) >= L or not used[r + 1:min(L, r + 1 + k)].any()
            if left_ok and right_ok:
                used[l:r + 1] = True
                covered = int(used.sum())
        trials.append(n)
    return mask, trials


def mask_span_1d(B, L, ratio, max_span, device):
    """HTR_VT.py:261-305: spans of 1 ... max_span tokens with the ratio-dependent spacing rule (k = span length up to a
    ratio of 0.4, 1 up to 0.7, 0 above) until round(ratio L) tokens are covered"""
    if ratio <= 0.0:
        return _zeros(B, L, device)
    return _upload(_span_host(B, L, ratio, max_span)[0], device)


def mask_span_old_1d(B, L, ratio, max_span, device):
    """HTR_VT.py:307-323: int(L ratio) // max_span spans of the fixed length min(max_span, L), the same starts for every
    sample.  The starts come from the device generator, one draw and one .item() per span, as in the fork."""
    if ratio <= 0.0 or max_span <= 0 or L <= 0:
        return _zeros(B, L, device)
    num_spans = int(L * ratio) // max(1, max_span)
    if num_spans <= 0:
        return _zeros(B, L, device)
    s = min(max_span, L)
    row = np.zeros(L, dtype=np.bool_)
    for _ in range(num_spans):
        start = torch.randint(0, L - s + 1, (1,), device=device).item()
        row[start:start + s] = True
    return _upload(np.tile(row, (B, 1)), device)


def generate_mms_mask(B, L, device, ratios=None, max_span_length=8, block_params=None):
    """HTR_VT.py:325-346: the union of a random, a block and a span mask as the float keep mask [B, L, 1] (1 keep /
    0 mask).  The random mask is drawn first (device generator), then block, then span (Python's generator); block and
    span are united on the host and uploaded together."""
    if ratios is None:
        ratios = DEFAULT_RATIOS
    min_block = int((block_params or {}).get("min_block", 2))
    m_rand = mask_random_1d(B, L, ratios.get("random", 0.50), device)
    r_block, r_span = ratios.get("block", 0.25), ratios.get("span", 0.25)
    host = np.zeros((B, L), dtype=np.bool_)
    if not r_block <= 0.0:
        host |= _block_host(B, L, r_block, min_block)[0]
    if not r_span <= 0.0:
        host |= _span_host(B, L, r_span, max_span_length)[0]
    return (~(m_rand | _upload(host, device))).float().unsqueeze(-1)


def keep_from_mask(mask):
    """bool [B, L] (True = masked) -> the forks' float keep mask [B, L, 1]"""
    return (~mask).float().unsqueeze(-1)
