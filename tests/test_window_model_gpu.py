"""Drop-in window-attention model on the MI355X against the reference fork run in float64 on the CPU
(tests/golden/window_model.npz, tools/make_goldens_window.py): eval logits, train-mode loss / gradients / BatchNorm
buffers with dropout off, the dropout refusal, reproducible Trainer steps, ModelEma and strict checkpoint loading."""
import copy
import os
from functools import partial

import numpy as np
import pytest
import torch

import window_cases as WC

pytestmark = pytest.mark.gpu


def _tiny(W, dtype=torch.float32, dropout=False):
    from htrvt_amd.window.model import HTR_VT as M
    torch.manual_seed(123)
    m = M.MaskedAutoencoderViT(WC.NB_CLS, img_size=[64, W], patch_size=(4, 64), embed_dim=256, depth=4, num_heads=4,
                               mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), compute_dtype=dtype,
                               dropout=dropout)
    WC.perturb(m)
    return m.cuda()


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "window_model.npz"))


@pytest.mark.parametrize("W", WC.TINY_WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_window_eval_logits(gold, W, dtype):
    m = _tiny(W, dtype).eval()
    x, _, _ = WC.tiny_batch(W)
    with torch.no_grad():
        y = m(x.cuda()).cpu().numpy()
    e = _rel(y, gold[f"tiny.{W}.eval"])
    print(f"W={W} {dtype}: eval logits rel-to-max {e:.3e}")
    assert e < (1e-3 if dtype == torch.float32 else 5e-2), e


def test_window_d768_eval_logits(gold):
    from htrvt_amd.window.model import HTR_VT as M
    torch.manual_seed(123)
    m = M.create_model(80, (64, 512)).cuda().eval()
    with torch.no_grad():
        y = m(WC.d768_images().cuda()).cpu().numpy()
    e = _rel(y, gold["d768.eval"])
    print(f"d768 N=128 eval logits rel-to-max {e:.3e}")
    assert e < 1e-3, e


@pytest.mark.parametrize("W", WC.TINY_WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_window_train_step_against_reference(gold, W, dtype):
    import htrvt_amd
    m = _tiny(W, dtype).train()
    x, tg, ln = WC.tiny_batch(W)
    torch.manual_seed(WC.MASK_SEED)
    y = m(x.cuda(), WC.MASK_RATIO, WC.MAX_SPAN, use_masking=True)
    loss = htrvt_amd.ctc_loss(y, tg, ln)
    loss.backward()
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    ref_loss = float(gold[f"tiny.{W}.loss"])
    assert abs(loss.item() - ref_loss) < (1e-4 if f32 else 3e-2) * abs(ref_loss), (loss.item(), ref_loss)
    assert _rel(y.detach().cpu().numpy(), gold[f"tiny.{W}.train"]) < (1e-3 if f32 else 5e-2)
    tol = 2e-3 if f32 else 1e-1
    worst = 0.0
    for n, p in m.named_parameters():
        g = p.grad.detach().cpu().numpy().ravel().astype(np.float64)
        if f"tiny.{W}.grad.{n}" in gold:
            want = gold[f"tiny.{W}.grad.{n}"]
            got = g
        else:
            want = gold[f"tiny.{W}.gsample.{n}"]
            got = g[WC.sample_index(g.size)]
            nr = float(gold[f"tiny.{W}.gnorm.{n}"])
            assert abs(np.linalg.norm(g) - nr) <= (1e-2 if f32 else 1e-1) * nr, n
        if n.startswith("patch_embed."):
            # the stem: a train-mode BatchNorm over two images and ReLU / max-pool arg-max discontinuities -- gated on the
            # sampled entries' cosine and the whole tensor's norm (above), as smoke() gates the stem of the v1 model
            cos = float(got @ want / (np.linalg.norm(got) * np.linalg.norm(want) + 1e-30))
            assert cos > (0.9999 if f32 else 0.9), (n, cos)    # bf16: the stem is reported, not gated tightly
            continue
        e = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))
        worst = max(worst, e)
        assert e < tol, (n, e)
    assert "blocks.0.attn.relative_position_bias_table" in dict(m.named_parameters())
    print(f"W={W} {dtype}: loss {loss.item():.5f} (ref {ref_loss:.5f}), worst gradient rel-to-max {worst:.2e}")
    if f32:
        for n, b in m.named_buffers():
            if "running" in n:
                np.testing.assert_allclose(b.cpu().numpy(), gold[f"tiny.{W}.buf.{n}"], rtol=1e-4, atol=1e-5, err_msg=n)


def test_window_train_forward_with_dropout_raises():
    m = _tiny(256, dropout=True).train()
    x, _, _ = WC.tiny_batch(256)
    with pytest.raises(NotImplementedError, match="dropout"):
        m(x.cuda())
    m.eval()
    with torch.no_grad():
        m(x.cuda())               # dropout is identity in eval mode: the fork's valid / test scripts run


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_window_trainer_step_bitwise_reproducible(dtype):
    from htrvt_amd.trainer import Trainer
    x, tg, ln = WC.tiny_batch(800)
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
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_window_ema_and_strict_load():
    import htrvt_amd
    m = _tiny(256)
    ema = htrvt_amd.ModelEma(m, 0.9)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01)
    ema.update(m)
    e = ema.ema
    t0 = m.state_dict()["blocks.0.attn.relative_position_bias_table"]
    te = e.state_dict()["blocks.0.attn.relative_position_bias_table"]
    assert torch.allclose(te, t0 - 0.009, atol=1e-5)
    m2 = _tiny(256)
    m2.load_state_dict(copy.deepcopy(m.state_dict()), strict=True)
    x, _, _ = WC.tiny_batch(256)
    m.eval(), m2.eval()
    with torch.no_grad():
        assert torch.equal(m(x.cuda()), m2(x.cuda()))
