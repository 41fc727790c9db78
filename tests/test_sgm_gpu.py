"""The SGM drop-in on the MI355X: the context batch, the head (float32 / bfloat16) and model_sgm_2's encoder with the
feature tap against the reference run in float64 on the CPU (tests/golden/sgm.npz, tools/make_goldens_sgm.py), and the head at 600 query rows
(three chunks of the query backward) against tests/sgm_refs.py in float64; padding,
the dropout generator, bitwise reproducibility and SAM-style `p.data` rebinding."""
import functools
import os
from functools import partial

import numpy as np
import pytest
import torch

import sgm_cases as C
import sgm_refs as R
from htrvt_amd._lib import lib
from htrvt_amd.ops import ptr, stream

pytestmark = pytest.mark.gpu


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sgm.npz"))


def _head(case, dtype, p_drop=0.1):
    from htrvt_amd.sgm.model.sgm_head import SGMHead
    B, L, N, D, dtx, V, S = C.HEAD_CASES[case]
    seed, _, vis = C.head_inputs(case)
    torch.manual_seed(seed)
    h = SGMHead(D, V, d_txt=dtx, sub_str_len=S, p_drop=p_drop, compute_dtype=dtype)
    C.perturb_head(h, seed)
    return h.cuda().eval(), vis.cuda()


def _ctx(g, pre):
    return [torch.from_numpy(g[pre + n]).cuda() for n in ("left", "right", "tgt", "mask")]


def _run(h, vis, ctx):
    v = vis.clone().requires_grad_(True)
    for p in h.parameters():
        p.grad = None
    out = h(v, *ctx)
    out["loss_sgm"].backward()
    grads = {n: p.grad.clone() for n, p in h.named_parameters()}
    grads["vis"] = v.grad.clone()
    return out, grads


def _cmp(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    e = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
    cos = float(got @ want / max(np.linalg.norm(got) * np.linalg.norm(want), 1e-30))
    return e, cos


def test_sgm_context_batch_bitwise(golden_dir):
    from htrvt_amd.sgm.model.sgm_head import build_sgm_vocab, make_context_batch
    g = _golden(golden_dir)
    stoi = build_sgm_vocab(C.Converter())[0]
    for key, texts in (("ctx", C.CONTEXT_TEXTS), ("ctx0", ["", ""])):
        got = make_context_batch(texts, stoi, 5, device="cuda")
        for n, t in zip(("left", "right", "tgt", "mask"), got):
            want = g[f"{key}.{n}"]
            assert t.is_cuda and t.dtype == torch.from_numpy(want).dtype and tuple(t.shape) == want.shape, (key, n)
            assert np.array_equal(t.cpu().numpy(), want), (key, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ["small", "d768"])
def test_sgm_head_against_reference(golden_dir, dtype, case):
    g = _golden(golden_dir)
    pre = f"head.{case}."
    h, vis = _head(case, dtype)
    out, grads = _run(h, vis, _ctx(g, pre))
    f32 = dtype == torch.float32
    loss = float(out["loss_sgm"])
    assert out["loss_sgm"].shape == () and out["loss_sgm"].dtype == torch.float32
    assert abs(loss - float(g[pre + "loss"])) <= (1e-5 if f32 else 1e-2) * abs(float(g[pre + "loss"])), loss
    for n in ("logits_l", "logits_r"):
        t = out[n]
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == g[pre + n].shape
        e, cos = _cmp(t.detach().cpu().numpy(), g[pre + n])
        print(f"{case} {dtype} {n}: rel-to-max {e:.3e} cosine {cos:.7f}")
        assert e < (3e-5 if f32 else 3e-2) and cos > (0.99999 if f32 else 0.999), (n, e, cos)
    for n, t in grads.items():
        a = t.cpu().numpy()
        if case == "small":
            e, cos = _cmp(a, g[pre + "grad." + n])
        else:
            idx = g[pre + "gidx." + n]
            got = a.reshape(-1)[idx]
            e = float(np.abs(got - g[pre + "gval." + n]).max() / float(g[pre + "gmax." + n]))
            _, cos = _cmp(got, g[pre + "gval." + n])
            rn = abs(float(np.linalg.norm(a)) / float(g[pre + "gnorm." + n]) - 1)
            assert rn < (2e-4 if f32 else 4e-2), (n, rn)
        print(f"{case} {dtype} grad {n}: rel-to-max {e:.3e} cosine {cos:.7f}")
        assert e < (2e-4 if f32 else 4e-2) and cos > (0.99999 if f32 else 0.999), (n, e, cos)


MULTI_CHUNK = (6, 50, 32, 64, 40, 30, 5)      # (B, L, N, D, d_txt, V, S): R = 2 B L = 600 rows, three chunks of the query backward


@functools.lru_cache(maxsize=None)
def _multi_chunk_reference():
    """tests/sgm_refs.head in float64 under autograd, once for both dtypes: (ctx, vis, head seed, loss, logits, gradients)"""
    B, L, N, D, dtx, V, S = MULTI_CHUNK
    stoi = C.vocab_for(V)
    ids = [[stoi[ch] for ch in t] for t in C.random_texts(B, L, V, seed=61)]
    ctx = R.context_batch(ids, S, stoi["<pad>"], stoi["<bos_left>"], stoi["<eos>"])
    vis = C.vis_tokens(B, N, D, seed=N + D + 1)
    h = _new_head(MULTI_CHUNK, torch.float32, 161)
    params = {n: p.detach().double().requires_grad_(True) for n, p in h.named_parameters()}
    v = vis.double().requires_grad_(True)
    loss, ll, lr = R.head(params, v, *ctx)
    loss.backward()
    grads = {n: p.grad.numpy() for n, p in params.items()}
    grads["vis"] = v.grad.numpy()
    return ctx, vis, loss.item(), {"logits_l": ll.detach().numpy(), "logits_r": lr.detach().numpy()}, grads


def _new_head(shape, dtype, seed):
    from htrvt_amd.sgm.model.sgm_head import SGMHead
    B, L, N, D, dtx, V, S = shape
    torch.manual_seed(seed)
    h = SGMHead(D, V, d_txt=dtx, sub_str_len=S, compute_dtype=dtype)
    C.perturb_head(h, seed)
    return h


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sgm_head_multi_chunk_against_float64(dtype):
    """the head where the query backward sums three chunks (the golden cases stay inside one), the gates of
    test_sgm_head_against_reference"""
    from htrvt_amd.sgm.model.sgm_head import make_context_batch
    B, L, N, D, dtx, V, S = MULTI_CHUNK
    ctx, vis, loss_ref, logits_ref, grads_ref = _multi_chunk_reference()
    assert ctx[0].shape == (B, L, S) and 2 * B * L == 600
    dev_ctx = make_context_batch(C.random_texts(B, L, V, seed=61), C.vocab_for(V), S)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(dev_ctx, ctx))
    h = _new_head(MULTI_CHUNK, dtype, 161).cuda().eval()
    out, grads = _run(h, vis.cuda(), dev_ctx)
    f32 = dtype == torch.float32
    loss = float(out["loss_sgm"])
    print(f"multi-chunk {dtype} loss {loss:.7f} float64 {loss_ref:.7f}")
    assert abs(loss - loss_ref) <= (1e-5 if f32 else 1e-2) * abs(loss_ref), loss
    for n in ("logits_l", "logits_r"):
        e, cos = _cmp(out[n].detach().cpu().numpy(), logits_ref[n])
        print(f"multi-chunk {dtype} {n}: rel-to-max {e:.3e} cosine {cos:.7f}")
        assert e < (3e-5 if f32 else 3e-2) and cos > (0.99999 if f32 else 0.999), (n, e, cos)
    assert set(grads) == set(grads_ref)
    for n, t in grads.items():
        e, cos = _cmp(t.cpu().numpy(), grads_ref[n])
        print(f"multi-chunk {dtype} grad {n}: rel-to-max {e:.3e} cosine {cos:.7f}")
        assert e < (2e-4 if f32 else 4e-2) and cos > (0.99999 if f32 else 0.999), (n, e, cos)
    out2, grads2 = _run(h, vis.cuda(), dev_ctx)
    assert torch.equal(out["loss_sgm"], out2["loss_sgm"])
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sgm_padding_has_no_gradient(golden_dir, dtype):
    g = _golden(golden_dir)
    h, vis = _head("small", dtype)
    ctx = _ctx(g, "head.small.")
    out, grads = _run(h, vis, ctx)
    pad = ctx[3] == 0
    assert bool(pad.any())
    gen = torch.Generator(device="cuda").manual_seed(5)
    scrambled = [c.clone() for c in ctx]
    for c in scrambled[:3]:                      # other ids at the padded positions: nothing may change
        r = torch.randint(0, 20, c.shape, device="cuda", generator=gen)
        m = pad if c.dim() == 2 else pad[..., None].expand_as(c)
        c[m] = r[m]
    out2, grads2 = _run(h, vis, scrambled)
    assert torch.equal(out["loss_sgm"], out2["loss_sgm"])
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n
    # an all-empty batch: loss 0, zero gradients
    from htrvt_amd.sgm.model.sgm_head import make_context_batch
    e = make_context_batch(["", "", ""], C.vocab_for(20), 5)
    out0, grads0 = _run(h, vis, e)
    assert float(out0["loss_sgm"]) == 0.0 and out0["logits_l"].shape == (3, 0, 20)
    for n, t in grads0.items():
        assert torch.isfinite(t).all() and not t.any(), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sgm_dropout_kernel(dtype):
    p, n = 0.1, 10_000_000 // 8 * 8
    dti = 0 if dtype == torch.float32 else 1
    x = (torch.rand(n, device="cuda") + 0.5).to(dtype)
    seed = torch.tensor([1234567], dtype=torch.int64, device="cuda")
    y, y2 = torch.empty_like(x), torch.empty_like(x)
    assert lib.htrvt_sgm_dropout(ptr(x), ptr(y), n, ptr(seed), p, dti, stream()) == 0
    assert lib.htrvt_sgm_dropout(ptr(x), ptr(y2), n, ptr(seed), p, dti, stream()) == 0
    assert torch.equal(y, y2)
    kept = y != 0
    frac = kept.double().mean().item()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(frac - (1 - p)) < 6 * sigma, frac
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    assert torch.equal(y[kept], (x[kept].float() * scale.cuda()).to(dtype))
    dy = torch.ones_like(x)
    dx = torch.empty_like(x)
    assert lib.htrvt_sgm_dropout(ptr(dy), ptr(dx), n, ptr(seed), p, dti, stream()) == 0
    assert torch.equal(dx != 0, kept)
    other = torch.tensor([7654321], dtype=torch.int64, device="cuda")
    assert lib.htrvt_sgm_dropout(ptr(x), ptr(y2), n, ptr(other), p, dti, stream()) == 0
    assert not torch.equal(y, y2)


def test_sgm_head_train_mode_dropout(golden_dir):
    g = _golden(golden_dir)
    ctx = _ctx(g, "head.small.")
    h0, vis = _head("small", torch.float32, p_drop=0.0)
    ev, gev = _run(h0, vis, ctx)
    tr, gtr = _run(h0.train(), vis, ctx)              # p = 0 in train mode: identity
    assert torch.equal(ev["loss_sgm"], tr["loss_sgm"]) and all(torch.equal(gev[n], gtr[n]) for n in gev)
    h, _ = _head("small", torch.float32, p_drop=0.1)
    h.train()
    cpu_state = torch.get_rng_state()
    torch.cuda.manual_seed(3)
    a, ga = _run(h, vis, ctx)
    torch.cuda.manual_seed(3)
    b, gb = _run(h, vis, ctx)
    assert torch.equal(cpu_state, torch.get_rng_state())       # the CPU stream (span masks) is untouched
    assert torch.equal(a["loss_sgm"], b["loss_sgm"]) and all(torch.equal(ga[n], gb[n]) for n in ga)
    c, _ = _run(h, vis, ctx)
    assert not torch.equal(a["logits_l"], c["logits_l"])
    assert not torch.equal(a["logits_l"], ev["logits_l"]) and all(torch.isfinite(t).all() for t in ga.values())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sgm_head_reproducible_and_rebinding(golden_dir, dtype):
    g = _golden(golden_dir)
    ctx = _ctx(g, "head.d768.")
    h, vis = _head("d768", dtype)
    a, ga = _run(h, vis, ctx)
    b, gb = _run(h, vis, ctx)
    assert torch.equal(a["loss_sgm"], b["loss_sgm"])
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    # SAM rebinds parameters through p.data: the next call must use the new values
    old = [p.data for p in h.parameters()]
    for p in h.parameters():
        p.data = p.data + 0.01 * torch.randn_like(p.data)
    c, _ = _run(h, vis, ctx)
    assert not torch.equal(a["loss_sgm"], c["loss_sgm"])
    for p, o in zip(h.parameters(), old):
        p.data = o
    d, _ = _run(h, vis, ctx)
    assert torch.equal(a["loss_sgm"], d["loss_sgm"])


def _tiny_model(dtype=torch.float32):
    from oracle import htrvt_oracle as O
    from htrvt_amd.sgm.model import HTR_VT as M
    cfg = O.Config(80, (64, 512), embed_dim=64, depth=2, num_heads=2)
    sd = O.init_state_dict(cfg, seed=7, randomize_affine=True)
    m = M.MaskedAutoencoderViT(80, img_size=[64, 512], patch_size=(4, 64), embed_dim=64, depth=2, num_heads=2, mlp_ratio=4,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def test_sgm_model_features_and_combined_loss(golden_dir):
    from htrvt_amd.sgm.model.sgm_head import SGMHead, make_context_batch
    g = _golden(golden_dir)
    t = np.load(os.path.join(golden_dir, "tiny_model.npz"))
    m = _tiny_model().train()
    x = torch.from_numpy(t["x"]).cuda()
    keep = torch.from_numpy(t["keep_mask"])
    with torch.no_grad():
        y0 = m(x, keep_mask=keep)
    m.load_state_dict(_tiny_model().state_dict())          # BatchNorm buffers back to the start
    logits, feats = m(x, keep_mask=keep, return_features=True)
    assert torch.equal(logits.detach(), y0)                 # bitwise the logits of a call without features
    assert feats.shape == (4, 128, 64) and feats.dtype == torch.float32 and feats.requires_grad
    e, cos = _cmp(feats.detach().cpu().numpy(), g["model.feats"])
    assert e < 1e-4 and cos > 0.99999, (e, cos)
    lp = logits.float().permute(1, 0, 2).log_softmax(2)
    crit = torch.nn.CTCLoss(reduction="none", zero_infinity=True)
    ctc = crit(lp, torch.from_numpy(t["targets"]).cuda(), torch.IntTensor([128] * 4).cuda(),
               torch.from_numpy(t["lengths"]).cuda()).mean()
    torch.manual_seed(77)
    head = SGMHead(64, 84, d_txt=32)
    C.perturb_head(head, 77)
    head = head.cuda().eval()
    ctx = make_context_batch(C.random_texts(4, 30, 84, seed=4), C.vocab_for(84), 5)
    sgm = head(feats, *ctx)["loss_sgm"]
    assert abs(float(sgm) - float(g["model.sgm"])) < 1e-4 * abs(float(g["model.sgm"]))
    (ctc + 1.0 * sgm).backward()
    params = dict(m.named_parameters())
    for k in g.files:
        if k.startswith("model.grad."):
            e, cos = _cmp(params[k[11:]].grad.cpu().numpy(), g[k])
            print(f"model grad {k[11:]}: rel-to-max {e:.3e} cosine {cos:.7f}")
            assert e < 2e-3 and cos > 0.9999, (k, e, cos)


def test_sgm_model_features_only_no_grad_and_split():
    from htrvt_amd.sgm.model import HTR_VT as M
    t = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_model.npz"))
    x = torch.from_numpy(t["x"]).cuda()
    m = _tiny_model().train()
    feats = m.forward_features(x, 0.4, 8, use_masking=True)
    (feats.square().mean()).backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    assert not grads["head.weight"].any() and not grads["head.bias"].any()       # the logits carry no loss
    assert grads["norm.weight"].abs().sum() > 0 and grads["blocks.0.attn.qkv.weight"].abs().sum() > 0
    assert all(torch.isfinite(v).all() for v in grads.values())
    with torch.no_grad():
        y, f = m(x, return_features=True)
    assert not y.requires_grad and not f.requires_grad
    mb = _tiny_model(torch.bfloat16).eval()
    with torch.no_grad():
        yb, fb = mb(x, return_features=True)
    assert fb.dtype == torch.float32 and fb.shape == (4, 128, 64) and torch.isfinite(fb).all()
    ms = M.create_model(80, (64, 512), compute_dtype="split_bf16").cuda().eval()
    with pytest.raises(NotImplementedError, match="split_bf16"):
        ms(torch.zeros(1, 1, 64, 512, device="cuda"), return_features=True)
