"""Drop-in LGP model on the MI355X against the reference fork run in float64 on the CPU (tests/golden/lgp_model.npz,
tools/make_goldens_lgp.py): eval logits, train-mode loss / gradients / BatchNorm buffers, reproducible Trainer steps,
ModelEma and strict checkpoint loading, and the calls of the fork's own training loop (train mode does not raise: the
fork has no dropout).  Gates: those of tests/test_window_model_gpu.py for the same tiny geometry."""
import copy
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

import lgp_cases as LC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(W, dtype=torch.float32):
    from htrvt_amd.lgp.model import HTR_VT as M
    torch.manual_seed(123)
    m = M.MaskedAutoencoderViT(LC.NB_CLS, img_size=[64, W], patch_size=(4, 64), embed_dim=256, depth=4, num_heads=4,
                               mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), compute_dtype=dtype)
    LC.perturb(m)
    return m.cuda()


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "lgp_model.npz"))


@pytest.mark.parametrize("W", LC.TINY_WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lgp_eval_logits(gold, W, dtype):
    m = _tiny(W, dtype).eval()
    x, _, _ = LC.tiny_batch(W)
    with torch.no_grad():
        y = m(x.cuda()).cpu().numpy()
    e = _rel(y, gold[f"tiny.{W}.eval"])
    print(f"W={W} {dtype}: eval logits rel-to-max {e:.3e}")
    assert e < (1e-3 if dtype == torch.float32 else 5e-2), e


def test_lgp_d768_eval_logits(gold):
    from htrvt_amd.lgp.model import HTR_VT as M
    torch.manual_seed(123)
    m = M.create_model(80, (64, 512)).cuda().eval()
    with torch.no_grad():
        y = m(LC.d768_images().cuda()).cpu().numpy()
    e = _rel(y, gold["d768.eval"])
    print(f"d768 N=128 eval logits rel-to-max {e:.3e}")
    assert e < 1e-3, e


@pytest.mark.parametrize("W", LC.TINY_WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lgp_train_step_against_reference(gold, W, dtype):
    import htrvt_amd
    m = _tiny(W, dtype).train()
    x, tg, ln = LC.tiny_batch(W)
    torch.manual_seed(LC.MASK_SEED)
    y = m(x.cuda(), LC.MASK_RATIO, LC.MAX_SPAN, use_masking=True)          # train mode runs: the point of this fork
    loss = htrvt_amd.ctc_loss(y, tg, ln)
    loss.backward()
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    ref_loss = float(gold[f"tiny.{W}.loss"])
    el = abs(loss.item() - ref_loss) / abs(ref_loss)
    ey = _rel(y.detach().cpu().numpy(), gold[f"tiny.{W}.train"])
    print(f"W={W} {dtype}: loss {loss.item():.5f} (ref {ref_loss:.5f}, rel {el:.2e}), train logits rel-to-max {ey:.2e}")
    tol = 2e-3 if f32 else 1e-1
    worst, fails = 0.0, []
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        g = p.grad.detach().cpu().numpy().ravel().astype(np.float64)
        if f"tiny.{W}.grad.{n}" in gold:
            want = gold[f"tiny.{W}.grad.{n}"]
            got = g
        else:
            want = gold[f"tiny.{W}.gsample.{n}"]
            got = g[LC.sample_index(g.size)]
            nr = float(gold[f"tiny.{W}.gnorm.{n}"])       # the whole tensor's norm: a sample cannot hide a wrong region
            en = abs(np.linalg.norm(g) - nr) / nr
            if en > (1e-2 if f32 else 1e-1):
                fails.append((n, "norm", en))
        if n.startswith("patch_embed."):
            # the stem: a train-mode BatchNorm over two images and ReLU / max-pool arg-max discontinuities -- gated on the
            # sampled entries' cosine and the whole tensor's norm (above), as smoke() gates the stem of the v1 model
            cos = float(got @ want / (np.linalg.norm(got) * np.linalg.norm(want) + 1e-30))
            if not cos > (0.9999 if f32 else 0.9):
                fails.append((n, "cosine", cos))
            continue
        e = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))
        if n.endswith("logit_alpha") or "qkv.bias" in n or e > 0.5 * tol:
            print(f"   {n}: rel-to-max {e:.2e}")
        worst = max(worst, e)
        # bfloat16 d logit_alpha of block 0 at W = 800: one scalar = a sum over B N D products of bfloat16-rounded tensors that
        # cancels to 1/1455 of its terms there (blocks 1-3: 1/12 ... 1/80), gated on its plain relative error (a one-element
        # tensor's maximum is itself).  Measured 0.224 (float32: 1.1e-3 on the same scalar against <= 5e-5 on every other
        # tensor); gate 0.3 for THIS scalar only, within twice its measured value; all others keep 0.1
        wide = not f32 and W == 800 and n == "blocks.0.global_attn.logit_alpha"
        if not e < (0.3 if wide else tol):
            fails.append((n, "rel-to-max", e))
    print(f"   worst encoder / head gradient rel-to-max {worst:.2e}")
    assert el < (1e-4 if f32 else 3e-2), (loss.item(), ref_loss)
    assert ey < (1e-3 if f32 else 5e-2), ey
    assert not fails, fails
    if f32:
        for n, b in m.named_buffers():
            if "running" in n:
                np.testing.assert_allclose(b.cpu().numpy(), gold[f"tiny.{W}.buf.{n}"], rtol=1e-4, atol=1e-5, err_msg=n)


def test_lgp_d768_bfloat16_step_against_float32_engine():
    """the full-size bfloat16 path -- the only place the block's strided launches (local proj with ldc = 2D, the dgrad /
    weight gradient / bias column sum reading one half of the [B N][2D] gradient) reach the 256-row kernel families --
    against the float32 engine of the same build on the same weights and batch: the project's bfloat16 gates (logits 5e-2,
    loss 3e-2, encoder / head gradients 1e-1 of the tensor's maximum and norm within 1e-1, stem by cosine 0.9).  The four
    d logit_alpha scalars are gated together as one four-element tensor (relative to the largest of them)."""
    import htrvt_amd
    from htrvt_amd.lgp.model import HTR_VT as M
    B = 4
    g = torch.Generator().manual_seed(12)
    img = torch.rand(B, 1, 64, 1024, generator=g).cuda()
    ln = torch.tensor([9, 14, 5, 11], dtype=torch.int32)
    tg = torch.randint(1, 80, (int(ln.sum()),), generator=g, dtype=torch.int32)
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(123)
        m = M.create_model(80, (64, 1024), compute_dtype=dtype)
        LC.perturb(m)
        m = m.cuda().train()
        torch.manual_seed(LC.MASK_SEED)
        y = m(img, LC.MASK_RATIO, LC.MAX_SPAN, use_masking=True)
        loss = htrvt_amd.ctc_loss(y, tg, ln)
        loss.backward()
        torch.cuda.synchronize()
        res[dtype] = (y.detach().cpu().numpy(), loss.item(), {n: p.grad.detach().double().cpu().numpy().ravel()
                                                              for n, p in m.named_parameters()})
        del m
    (y32, l32, g32), (y16, l16, g16) = res[torch.float32], res[torch.bfloat16]
    ey, el = _rel(y16, y32), abs(l16 - l32) / abs(l32)
    print(f"d768 N=256 B={B}: logits rel-to-max {ey:.2e}, loss {l16:.4f} vs {l32:.4f} (rel {el:.2e})")
    fails, worst = [], ("", 0.0)
    alphas = [n for n in g32 if n.endswith("logit_alpha")]
    amax = max(abs(g32[n][0]) for n in alphas)
    for n in g32:
        a, b = g16[n], g32[n]
        if n in alphas:
            e = abs(a[0] - b[0]) / amax
            print(f"   {n}: {a[0]:.4e} vs {b[0]:.4e}, {e:.2e} of the largest")
        elif n.startswith("patch_embed."):
            cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
            if not cos > 0.9:
                fails.append((n, "cosine", cos))
            continue
        else:
            e = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))
            en = abs(np.linalg.norm(a) - np.linalg.norm(b)) / np.linalg.norm(b)
            if not en < 1e-1:
                fails.append((n, "norm", en))
        if e > worst[1]:
            worst = (n, e)
        if not e < 1e-1:
            fails.append((n, "rel-to-max", e))
    print(f"   worst encoder / head gradient rel-to-max {worst[1]:.2e} ({worst[0]})")
    assert ey < 5e-2 and el < 3e-2, (ey, el)
    assert not fails, fails


def test_lgp_assigned_pos_embed_is_used_and_tall_images_are_refused():
    from htrvt_amd.lgp.model import HTR_VT as M
    m = _tiny(256).eval()
    x, _, _ = LC.tiny_batch(256)
    with torch.no_grad():
        y0 = m(x.cuda())
        m.pos_embed = torch.zeros_like(m.pos_embed)           # the fork's buffer, assigned by a caller
        y1 = m(x.cuda())
        m.pos_embed = torch.from_numpy(M.get_2d_sincos_pos_embed(256, (1, 64))).float().unsqueeze(0).cuda()
        y2 = m(x.cuda())
    assert not torch.equal(y0, y1) and torch.equal(y0, y2)
    m.pos_embed = torch.zeros(1, 63, 256, device="cuda")
    with pytest.raises(ValueError, match="pos_embed"):
        m(x.cuda())
    with pytest.raises(NotImplementedError, match="64-pixel"):
        M.create_model(80, (128, 512))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lgp_trainer_step_bitwise_reproducible(dtype):
    from htrvt_amd.trainer import Trainer
    x, tg, ln = LC.tiny_batch(800)
    runs = []
    for _ in range(2):
        m = _tiny(800, dtype)
        tr = Trainer(m, max_lr=1e-3, betas=(0.9, 0.99), weight_decay=0.5)
        losses = []
        for it in range(2):
            torch.manual_seed(40 + it)
            mask = m.generate_span_mask(m.tokens, 0.4, 8)
            losses.append(float(tr.step(x.cuda(), tg, ln, keep_mask=mask)))
        torch.cuda.synchronize()
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0]))
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    a0 = float(_tiny(800, dtype).blocks[2].global_attn.logit_alpha.detach())
    assert float(runs[0][1]["blocks.2.global_attn.logit_alpha"]) != a0          # the 0-dim parameter lives in the flat buffer
    with pytest.raises(NotImplementedError, match="capture_step"):
        tr.capture_step(x.cuda(), 16)


def test_lgp_ema_and_strict_load():
    import htrvt_amd
    m = _tiny(256)
    ema = htrvt_amd.ModelEma(m, 0.9)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01)
    ema.update(m)
    e = ema.ema
    t0 = m.state_dict()["blocks.0.global_attn.logit_alpha"]
    te = e.state_dict()["blocks.0.global_attn.logit_alpha"]
    assert te.dim() == 0 and torch.allclose(te, t0 - 0.009, atol=1e-5)
    assert "pos_embed" not in e.state_dict() and torch.equal(e.pos_embed, m.pos_embed)
    m2 = _tiny(256)
    m2.load_state_dict(copy.deepcopy(m.state_dict()), strict=True)
    x, _, _ = LC.tiny_batch(256)
    m.eval(), m2.eval()
    with torch.no_grad():
        assert torch.equal(m(x.cuda()), m2(x.cuda()))


def test_lgp_unserved_options_raise():
    m = _tiny(256).eval()
    eng = m._engine(torch.device("cuda"))
    x, _, _ = LC.tiny_batch(256)
    with pytest.raises(NotImplementedError, match="want_features"):
        eng.forward(dict(m.state_dict(keep_vars=True)), x.cuda(), want_features=True)
    from htrvt_amd.engine import Engine
    with pytest.raises(NotImplementedError, match="split_bf16"):
        Engine(m._shape, torch.float32, "cuda", split_bf16=True)


def test_lgp_fork_training_loop_calls():
    """the calls of the fork's train.py (:22, 58-68, 119-126) with its import layout: forward with the span mask, ATen
    log_softmax + CTCLoss, backward, a SAM-style perturbation that rebinds p.data between two passes, AdamW, ModelEma,
    then an eval / no_grad forward"""
    import htrvt_amd
    saved_path, saved_mods = list(sys.path), {k: v for k, v in sys.modules.items() if k == "model" or k.startswith("model.")}
    for k in saved_mods:
        del sys.modules[k]
    sys.path[:0] = [os.path.join(ROOT, "htr-vt_amd", "lgp"), ROOT]
    try:
        from model import HTR_VT
        assert HTR_VT.__file__.endswith(os.path.join("lgp", "model", "HTR_VT.py"))
        torch.manual_seed(1)
        model = HTR_VT.create_model(nb_cls=80, img_size=[64, 512])
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]
        sys.modules.update(saved_mods)
    model.train()
    model = model.cuda()
    model_ema = htrvt_amd.ModelEma(model, 0.9999)
    model.zero_grad()
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.99), weight_decay=0.5)
    criterion = torch.nn.CTCLoss(reduction="none", zero_infinity=True)
    g = torch.Generator().manual_seed(2)
    B = 2
    image = torch.rand(B, 1, 64, 512, generator=g).cuda()
    length = torch.tensor([5, 9], dtype=torch.int32)
    text = torch.randint(1, 80, (int(length.sum()),), generator=g, dtype=torch.int32)

    def compute_loss():
        preds = model(image, 0.4, 8, use_masking=True).float()
        preds_size = torch.IntTensor([preds.size(1)] * B).cuda()
        preds = preds.permute(1, 0, 2).log_softmax(2)
        return criterion(preds, text.cuda(), preds_size, length.cuda()).mean()

    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss = compute_loss()
    loss.backward()
    assert all(p.grad is not None for p in model.parameters())
    # SAM.first_step: e_w = rho g / |g|, p.data rebound; second pass at the perturbed point; SAM.second_step restores
    gn = torch.norm(torch.stack([p.grad.norm(2) for p in model.parameters()]), 2)
    old = {}
    for p in model.parameters():
        old[p] = p.data.clone()
        p.data = p.data + 0.05 * p.grad / (gn + 1e-12)
    optimizer.zero_grad()
    loss2 = compute_loss()
    loss2.backward()
    for p in model.parameters():
        p.data = old[p]
    optimizer.step()
    model.zero_grad()
    model_ema.update(model)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and np.isfinite(loss2.item()) and loss.item() != loss2.item()
    changed = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(changed) == len(before), sorted(set(before) - set(changed))
    model.eval()
    with torch.no_grad():
        y = model(image)
    assert y.shape == (B, 128, 80) and bool(torch.isfinite(y).all())
