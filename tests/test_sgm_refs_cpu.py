"""tests/sgm_refs.py, the yardstick of tests/test_sgm_kernels_gpu.py, anchored without a GPU: its context batch against
the reference's (tests/golden/sgm.npz, bit for bit), its head in float64 against the reference head's float64 run stored
there (the goldens are float32 arrays: half an ulp, 6e-8, of rounding), and its two hand-written backward statements
against float64 autograd of the forward ones."""
import os

import numpy as np
import pytest
import torch

import sgm_cases as C
import sgm_refs as S

F64 = torch.float64


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sgm.npz"))


def _ids(texts, stoi):
    return [[stoi[ch] for ch in t] for t in texts]


def test_context_batch_matches_reference_bitwise(golden_dir):
    from htrvt_amd.sgm.model.sgm_head import build_sgm_vocab
    g = _golden(golden_dir)
    stoi, _, pad, eos, bos_l, _ = build_sgm_vocab(C.Converter())
    for key, texts in (("ctx", C.CONTEXT_TEXTS), ("ctx0", ["", ""])):
        got = S.context_batch(_ids(texts, stoi), 5, pad, bos_l, eos)
        for n, t in zip(("left", "right", "tgt", "mask"), got):
            want = g[f"{key}.{n}"]
            assert t.dtype == torch.from_numpy(want).dtype and tuple(t.shape) == want.shape, (key, n)
            assert np.array_equal(t.numpy(), want), (key, n)
    # the head case's batch too: other lengths, another vocabulary
    B, L, N, D, dtx, V, Sw = C.HEAD_CASES["small"]
    stoi = C.vocab_for(V)
    got = S.context_batch(_ids(C.head_inputs("small")[1], stoi), Sw, stoi["<pad>"], stoi["<bos_left>"], stoi["<eos>"])
    for n, t in zip(("left", "right", "tgt", "mask"), got):
        assert np.array_equal(t.numpy(), g["head.small." + n]), n


def test_head_float64_matches_reference_head(golden_dir):
    from htrvt_amd.sgm.model.sgm_head import SGMHead
    g = _golden(golden_dir)
    pre = "head.small."
    B, L, N, D, dtx, V, Sw = C.HEAD_CASES["small"]
    seed, _, vis = C.head_inputs("small")
    torch.manual_seed(seed)
    h = SGMHead(D, V, d_txt=dtx, sub_str_len=Sw)
    C.perturb_head(h, seed)
    params = {n: p.detach().double().requires_grad_(True) for n, p in h.named_parameters()}
    v = vis.double().requires_grad_(True)
    ctx = [torch.from_numpy(g[pre + n]) for n in ("left", "right", "tgt", "mask")]
    loss, ll, lr = S.head(params, v, *ctx)
    want = float(g[pre + "loss"])
    print(f"loss {loss.item():.17g} golden {want:.17g} rel {abs(loss.item() - want) / abs(want):.2e}")
    assert loss.dtype == F64 and abs(loss.item() - want) <= 1e-12 * abs(want)
    loss.backward()
    got = {"logits_l": ll.detach(), "logits_r": lr.detach(), "grad.vis": v.grad}
    got.update({"grad." + n: p.grad for n, p in params.items()})
    assert len(got) == 14
    for n, t in got.items():
        ref = torch.from_numpy(g[pre + n]).double()
        assert t.shape == ref.shape, n
        e = float((t - ref).abs().max() / ref.abs().max())
        print(f"{n}: {e:.2e} of max")
        assert e <= 1e-6, (n, e)


def _case(B, L, Sw, V, dtx, seed):
    gen = torch.Generator().manual_seed(seed)
    left = torch.randint(-2, V + 2, (B, L, Sw), generator=gen)
    right = torch.randint(-2, V + 2, (B, L, Sw), generator=gen)
    return gen, left, right


@pytest.mark.parametrize("B,L,Sw,V,dtx", [(1, 1, 1, 5, 3), (3, 7, 5, 11, 6), (2, 9, 4, 3, 8)])
def test_query_bwd_is_autograd_of_query_fwd(B, L, Sw, V, dtx):
    gen, left, right = _case(B, L, Sw, V, dtx, 7 * L + V)
    emb, dl, dr = (torch.randn(s, dtype=F64, generator=gen).requires_grad_(True) for s in ((V, dtx), (1, 1, dtx), (dtx,)))
    dq = torch.randn(B, 2, L, dtx, dtype=F64, generator=gen)
    q = S.query_fwd(left, right, emb, dl, dr)
    assert q.shape == (B, 2, L, dtx)
    # the statement itself: row (b, dir, l) is the mean of its S clamped embedding rows plus its direction's token
    b, l = B - 1, L - 1
    rows = emb.detach()[right[b, l].clamp(0, V - 1)]
    assert torch.allclose(q[b, 1, l].detach(), rows.mean(0) + dr.detach(), rtol=0, atol=1e-14)
    (q * dq).sum().backward()
    got = S.query_bwd(left, right, dq, V)
    for n, a, w in zip(("demb", "ddir_l", "ddir_r"), got, (emb.grad, dl.grad.reshape(-1), dr.grad)):
        assert a.shape == w.shape and float((a - w).abs().max()) <= 1e-12 * float(w.abs().max()), n


@pytest.mark.parametrize("V,ldv,B,L", [(1, 1, 1, 1), (5, 8, 2, 3), (20, 24, 3, 7), (65, 65, 1, 4)])
@pytest.mark.parametrize("mask_kind", ["ones", "mixed", "zero"])
def test_xent_bwd_is_autograd_of_xent_fwd(V, ldv, B, L, mask_kind):
    gen = torch.Generator().manual_seed(V + L)
    R = 2 * B * L
    logits = (3 * torch.randn(R, ldv, dtype=F64, generator=gen)).requires_grad_(True)
    tgt = torch.randint(-2, V + 2, (B, L), generator=gen)
    mask = {"ones": torch.ones(B, L), "zero": torch.zeros(B, L),
            "mixed": (torch.rand(B, L, generator=gen) < 0.5).float()}[mask_kind].double()
    gout = torch.randn((), dtype=F64, generator=gen)
    dl_l, dl_r = torch.randn(B, L, V, dtype=F64, generator=gen), torch.randn(B, L, V, dtype=F64, generator=gen)
    lse, rowloss, loss, den = S.xent_fwd(logits, V, B, L, tgt, mask)
    assert float(den) == 2 * max(float(mask.sum()), 1.0)
    want = _torch_loss(logits.detach()[:, :V], V, B, L, tgt, mask)
    assert abs(loss.item() - want) <= 1e-12 * max(abs(want), 1.0)
    copies = logits.view(B, 2, L, ldv)[..., :V]
    (gout * loss + (copies[:, 0] * dl_l).sum() + (copies[:, 1] * dl_r).sum()).backward()
    got = S.xent_bwd(logits.detach(), V, B, L, tgt, mask, gout, dl_l, dl_r)
    assert got.shape == (R, ldv) and not got[:, V:].any()
    assert float((got - logits.grad).abs().max()) <= 1e-12 * float(logits.grad.abs().max())
    # the optional arguments: no loss gradient, no logits gradients
    only_loss = torch.autograd.grad(gout * S.xent_fwd(logits, V, B, L, tgt, mask)[2], logits)[0]
    assert float((S.xent_bwd(logits.detach(), V, B, L, tgt, mask, gout) - only_loss).abs().max()) <= 1e-12
    assert not S.xent_bwd(logits.detach(), V, B, L, tgt, mask).any()


def _torch_loss(x, V, B, L, tgt, mask):
    """torch's own operator, the way the head's docstring states the loss"""
    t = tgt.clamp(0, V - 1)
    x = x.view(B, 2, L, V)
    per = sum(torch.nn.functional.cross_entropy(x[:, d].reshape(-1, V), t.reshape(-1), reduction="none") for d in (0, 1))
    return float((per.view(B, L) * mask).sum() / (2.0 * mask.sum().clamp_min(1.0)))
