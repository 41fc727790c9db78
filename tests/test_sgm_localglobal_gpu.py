"""Drop-in SGM local-global model on the MI355X against the reference fork run in float64 on the CPU
(tests/golden/sgm_localglobal.npz, tools/make_goldens_sgm_localglobal.py): eval logits and features, train-mode logits /
features / loss with the seeded span mask, every parameter gradient of loss_ctc + sum(feats * R) (the feature tap's gradient
without the SGM head), BatchNorm buffers, and the determinism of a step of the fork's objective.

Gates, restated from where the project applies them to the same quantities -- tests/test_lgp_model_gpu.py: logits 1e-3
(bfloat16 5e-2) of the maximum, loss 1e-4 (3e-2), encoder / head gradients 2e-3 (1e-1) of the tensor's maximum, a sampled
tensor's norm 1e-2 (1e-1), the stem by cosine 0.9999 (0.9), BN buffers rtol 1e-4 atol 1e-5; tests/test_sgm_gpu.py: float32
features 1e-4 of the maximum with cosine > 0.99999."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import sgm_cases as C
import sgm_localglobal_cases as SC
from test_lgp_model_gpu import _rel
from test_sgm_gpu import _cmp

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _tiny(W, dtype=torch.float32):
    from htrvt_amd.sgm_localglobal.model import HTR_VT as M
    torch.manual_seed(123)
    m = M.MaskedAutoencoderViT(SC.NB_CLS, img_size=[64, W], patch_size=SC.TINY[W],
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), compute_dtype=dtype, **SC.TINY_KW)
    SC.perturb(m)
    return m.cuda()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "sgm_localglobal.npz"))


def _act(gold, key, got, what, rel_tol, cos_min=None):
    """an activation stored whole, or as the fixed sample + the whole tensor's norm"""
    got = got.detach().cpu().numpy().astype(np.float64)
    if key in gold:
        want, g = gold[key].ravel(), got.ravel()
    else:
        want, g = gold[key + ".s"], got.ravel()[SC.act_index(got.size)]
        nr = float(gold[key + ".n"])
        en = abs(np.linalg.norm(got) - nr) / nr
        assert en < rel_tol, (what, "norm", en)
    e, cos = _cmp(g, want)
    assert e == _rel(g, want.astype(np.float64))
    print(f"   {what}: rel-to-max {e:.3e} cosine {cos:.7f}")
    assert e < rel_tol, (what, e)
    if cos_min is not None:
        assert cos > cos_min, (what, cos)


@pytest.mark.parametrize("W", SC.TINY_WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_slg_eval_logits_and_features(gold, W, dtype):
    m = _tiny(W, dtype).eval()
    x, _, _ = SC.tiny_batch(W)
    with torch.no_grad():
        y0 = m(x.cuda())
        y, f = m(x.cuda(), return_features=True)
        f2 = m.forward_features(x.cuda())
    assert torch.equal(y, y0) and torch.equal(f, f2)        # bitwise the logits of a call without features
    assert f.shape == (2, W // 4, 256) and f.dtype == torch.float32
    f32 = dtype == torch.float32
    print(f"W={W} {dtype}")
    _act(gold, f"tiny.{W}.eval", y, "eval logits", 1e-3 if f32 else 5e-2)
    if f32:
        _act(gold, f"tiny.{W}.eval_feats", f, "eval features", 1e-4, 0.99999)


def test_slg_d768_eval_logits(gold):
    from htrvt_amd.sgm_localglobal.model import HTR_VT as M
    torch.manual_seed(123)
    m = M.create_model(80, (64, 512)).cuda().eval()
    with torch.no_grad():
        y = m(SC.d768_images().cuda()).cpu().numpy()
    e = _rel(y, gold["d768.eval"])
    print(f"d768 N=128 eval logits rel-to-max {e:.3e}")
    assert e < 1e-3, e


@pytest.mark.parametrize("W", SC.TINY_WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_slg_train_step_against_reference(gold, W, dtype):
    import htrvt_amd
    m = _tiny(W, dtype).train()
    x, tg, ln = SC.tiny_batch(W)
    torch.manual_seed(SC.MASK_SEED)
    y, f = m(x.cuda(), SC.MASK_RATIO, SC.MAX_SPAN, use_masking=True, return_features=True)
    loss = htrvt_amd.ctc_loss(y, tg, ln)
    R = SC.feature_weights(*f.shape).cuda()
    (loss + (f * R).sum()).backward()
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    ref_loss = float(gold[f"tiny.{W}.loss"])
    el = abs(loss.item() - ref_loss) / abs(ref_loss)
    print(f"W={W} {dtype}: loss {loss.item():.5f} (ref {ref_loss:.5f}, rel {el:.2e})")
    _act(gold, f"tiny.{W}.train", y, "train logits", 1e-3 if f32 else 5e-2)
    if f32:
        _act(gold, f"tiny.{W}.train_feats", f, "train features", 1e-4, 0.99999)
    assert el < (1e-4 if f32 else 3e-2), (loss.item(), ref_loss)
    tol = 2e-3 if f32 else 1e-1
    worst, fails, seen = 0.0, [], 0
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert n == "pos_embed" and p.grad is None
            continue
        assert p.grad is not None, n
        seen += 1
        g = p.grad.detach().cpu().numpy().ravel().astype(np.float64)
        if f"tiny.{W}.grad.{n}" in gold:
            want, got = gold[f"tiny.{W}.grad.{n}"], g
        else:
            want, got = gold[f"tiny.{W}.gsample.{n}"], g[SC.sample_index(g.size)]
            nr = float(gold[f"tiny.{W}.gnorm.{n}"])
            en = abs(np.linalg.norm(g) - nr) / nr
            if en > (1e-2 if f32 else 1e-1):
                fails.append((n, "norm", en))
        if n.startswith("patch_embed."):
            cos = float(got @ want / (np.linalg.norm(got) * np.linalg.norm(want) + 1e-30))
            if not cos > (0.9999 if f32 else 0.9):
                fails.append((n, "cosine", cos))
            continue
        e = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))
        if "qkv.bias" in n or e > 0.5 * tol:
            print(f"   {n}: rel-to-max {e:.2e}")
        worst = max(worst, e)
        if not e < tol:
            fails.append((n, "rel-to-max", e))
    print(f"   worst encoder / head gradient rel-to-max {worst:.2e}")
    assert seen == sum(1 for k in gold.files if k.startswith(f"tiny.{W}.grad.") or k.startswith(f"tiny.{W}.gsample."))
    assert f"tiny.{W}.grad.blocks.1.attn.qkv.bias" in gold          # carries dpad of the shifted block
    assert not fails, fails
    if f32:
        for n, b in m.named_buffers():
            if "running" in n:
                np.testing.assert_allclose(b.cpu().numpy(), gold[f"tiny.{W}.buf.{n}"], rtol=1e-4, atol=1e-5, err_msg=n)


def _objective_step(dtype):
    """one iteration of the fork's train.py objective (:37-63): ctc_lambda * CTC + sgm_lambda * SGM over the feature tap,
    model and head in train mode, AdamW over both"""
    from htrvt_amd.sgm.model.sgm_head import SGMHead, build_sgm_vocab, make_context_batch
    W = 800
    m = _tiny(W, dtype).train()
    stoi = build_sgm_vocab(C.Converter())[0]
    torch.manual_seed(9)
    head = SGMHead(256, len(stoi), d_txt=64, sub_str_len=5, compute_dtype=dtype).cuda().train()
    params = list(m.parameters()) + list(head.parameters())
    opt = torch.optim.AdamW([p for p in params if p.requires_grad], lr=1e-3, betas=(0.9, 0.99), weight_decay=0.5)
    crit = torch.nn.CTCLoss(reduction="none", zero_infinity=True)
    x, tg, ln = SC.tiny_batch(W)
    texts = C.random_texts(2, 12, 84, seed=3)
    torch.manual_seed(SC.MASK_SEED)
    torch.cuda.manual_seed(4)
    preds, feats = m(x.cuda(), SC.MASK_RATIO, SC.MAX_SPAN, use_masking=True, return_features=True)
    size = torch.IntTensor([preds.size(1)] * 2).cuda()
    ctc = crit(preds.float().permute(1, 0, 2).log_softmax(2), tg.cuda(), size, ln.cuda()).mean()
    sgm = head(feats, *make_context_batch(texts, stoi, sub_str_len=5, device=preds.device))["loss_sgm"]
    total = 0.1 * ctc + 1.0 * sgm
    total.backward()
    opt.step()
    torch.cuda.synchronize()
    return float(total), {n: p.detach().clone() for n, p in list(m.named_parameters()) + list(head.named_parameters())}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_slg_fork_objective_step_bitwise_reproducible(dtype):
    (l0, w0), (l1, w1) = _objective_step(dtype), _objective_step(dtype)
    assert np.isfinite(l0) and l0 == l1
    for n in w0:
        assert torch.equal(w0[n], w1[n]), n
    start = dict(_tiny(800, dtype).named_parameters())
    moved = [n for n in start if n != "pos_embed" and not torch.equal(start[n].detach(), w0[n])]
    assert len(moved) == len(start) - 1, sorted(set(start) - set(moved))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_slg_trainer_step_bitwise_reproducible(dtype):
    from htrvt_amd.trainer import Trainer
    x, tg, ln = SC.tiny_batch(800)
    runs = []
    for _ in range(2):
        m = _tiny(800, dtype)
        tr = Trainer(m, max_lr=1e-3, betas=(0.9, 0.99), weight_decay=0.5)
        losses = []
        for it in range(2):
            torch.manual_seed(40 + it)
            mask = m.generate_span_mask(m.num_patches, 0.4, 8)
            losses.append(float(tr.step(x.cuda(), tg, ln, keep_mask=mask)))
        torch.cuda.synchronize()
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0]))
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    b0 = _tiny(800, dtype).blocks[1].attn.qkv.bias.detach()
    assert not torch.equal(runs[0][1]["blocks.1.attn.qkv.bias"], b0)


def test_slg_unserved_options_raise():
    from htrvt_amd.engine import Engine
    m = _tiny(256)
    with pytest.raises(NotImplementedError, match="split_bf16"):
        Engine(m._shape, torch.float32, "cuda", split_bf16=True)
