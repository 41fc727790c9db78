"""Per-sample token masks on the MI355X (the multi-mask forks' keep [B, L, 1]): the per-sample token assembly
htrvt_pool_tokens_ps / htrvt_pool_tokens_bwd_ps against torch's max_pool2d autograd, their stride-0 call against the
shared-mask symbols, the stand-alone operator variants.mask_tokens against the forks' torch expression, and the mask's
way through Engine.forward, Trainer.step and GraphedStep.step.

Shapes of the assembly tests: B = 3, stem heights H in {1, 2, 3} (H = 2 takes the one-pooled-row backward), pooled rows
of W in {5, 66} tokens, i.e. N = W tokens for H = 1 and H = 2 and N = 2 W in {10, 132} for H = 3 (two pooled rows: an odd
N does not exist there, the entry points refuse N % 2 != 0); D in {8, 72} (bfloat16) / {4, 36} (float32).  The launches
cap their grid at 2048 blocks of 256 threads, so one more case runs 540 000 / 810 000 work items: past one grid-stride pass.
"""
import functools
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import dt, ptr, stream
    return lib, check, ptr, stream, dt


def _sample_masks(N):
    """[3, N]: sample 0 all kept, sample 1 all masked, sample 2 alternating with its first and last token masked"""
    keep = torch.ones(3, N)
    keep[1] = 0.0
    keep[2, 0::2] = 0.0
    keep[2, N - 1] = 0.0
    return keep


@functools.lru_cache(maxsize=None)
def _pool_case(H, W, D):
    """inputs and the float32 torch restatement (max_pool2d, select, + pos; autograd for the backward) of one shape, computed
    once for the tests that share it and not modified: (x NHWC, keep [3, N], mask_token, pos, dtok, tok_ref, dx_ref NHWC)"""
    B = 3
    g = torch.Generator().manual_seed(H * 1000 + W + D)
    Ho = (H - 1) // 2 + 1
    N = Ho * W
    # a per-(image, channel) permutation of 0..8 laid out with period 3 has a unique maximum in every (clipped) 3x3 window
    # and is exact in bfloat16, as are the small integers of pos, mask_token and dtok and every sum of them
    perm = torch.stack([torch.randperm(9, generator=g) for _ in range(B * D)]).view(B, D, 9).float()
    cell = (torch.arange(H).view(H, 1) % 3) * 3 + (torch.arange(W).view(1, W) % 3)
    x = perm[:, :, cell.view(-1)].view(B, D, H, W)
    keep = _sample_masks(N)
    mask_token = torch.randint(-7, -2, (D,), generator=g).float()
    pos = torch.randint(-4, 5, (N, D), generator=g).float()
    dtok = torch.randint(-8, 9, (B, N, D), generator=g).float()
    xr = x.clone().requires_grad_(True)
    pooled = torch.nn.functional.max_pool2d(xr, kernel_size=3, stride=(2, 1), padding=1)   # [B, D, Ho, W]
    k3 = keep.view(B, N, 1)
    tok_ref = pooled.permute(0, 2, 3, 1).reshape(B, N, D) * k3 + (1 - k3) * mask_token + pos
    (tok_ref * dtok).sum().backward()
    return (x.permute(0, 2, 3, 1).contiguous(), keep, mask_token, pos, dtok, tok_ref.detach(),
            xr.grad.permute(0, 2, 3, 1).contiguous())


POOL_SHAPES = [(H, W) for H in (1, 2, 3) for W in (5, 66)]
POOL_CASES = ([(H, W, D, torch.bfloat16) for H, W in POOL_SHAPES for D in (8, 72)]
              + [(H, W, D, torch.float32) for H, W in POOL_SHAPES for D in (4, 36)])


@pytest.mark.parametrize("H,W,D,dtype", POOL_CASES + [(3, 10000, 36, torch.float32)])
def test_per_sample_pool_tokens_and_backward_match_max_pool2d(H, W, D, dtype):
    """the comparison of test_pool_tokens_and_its_backward_match_max_pool2d (exact equality on data whose every value is
    exact in both dtypes) with one mask row per sample; a kernel that reads row 0 for every sample fails on samples 1, 2"""
    lib, check, ptr, stream, dt = _lib()
    x, keep, mask_token, pos, dtok, tok_ref, dx_ref = _pool_case(H, W, D)
    B, N = 3, keep.shape[1]
    x_d, keep_d, dtok_d = x.to(dtype).cuda(), keep.cuda(), dtok.to(dtype).cuda()
    mt_d, pos_d = mask_token.cuda(), pos.cuda()
    tok = torch.empty(B, N, D, dtype=dtype, device="cuda")
    check(lib.htrvt_pool_tokens_ps(ptr(x_d), ptr(keep_d), N, ptr(mt_d), ptr(pos_d), ptr(tok), B, H, N, D, dt(dtype), stream()),
          "pool_tokens_ps")
    assert torch.equal(tok.float().cpu(), tok_ref)
    dx = torch.empty(B, H, W, D, dtype=dtype, device="cuda")
    check(lib.htrvt_pool_tokens_bwd_ps(ptr(dtok_d), ptr(x_d), ptr(keep_d), N, ptr(dx), B, H, N, D, dt(dtype), stream()),
          "pool_tokens_bwd_ps")
    assert torch.equal(dx.float().cpu(), dx_ref)
    assert dx[1].count_nonzero() == 0 and dx[0].count_nonzero() > 0        # all masked / all kept


@pytest.mark.parametrize("H,W,D,dtype", POOL_CASES)
def test_stride_zero_equals_the_shared_mask_symbols_bitwise(H, W, D, dtype):
    lib, check, ptr, stream, dt = _lib()
    B = 3
    Ho = (H - 1) // 2 + 1
    N = Ho * W
    g = torch.Generator().manual_seed(H + W + D)
    x = torch.randn(B, H, W, D, generator=g).to(dtype).cuda()
    keep = (torch.rand(N, generator=g) > 0.4).float()
    keep[0], keep[N - 1] = 0.0, 1.0
    keep = keep.cuda()
    mt, pos = torch.randn(D, generator=g).cuda(), torch.randn(N, D, generator=g).cuda()
    dtok = torch.randn(B, N, D, generator=g).to(dtype).cuda()
    tok = [torch.empty(B, N, D, dtype=dtype, device="cuda") for _ in range(2)]
    dx = [torch.empty(B, H, W, D, dtype=dtype, device="cuda") for _ in range(2)]
    check(lib.htrvt_pool_tokens(ptr(x), ptr(keep), ptr(mt), ptr(pos), ptr(tok[0]), B, H, N, D, dt(dtype), stream()))
    check(lib.htrvt_pool_tokens_ps(ptr(x), ptr(keep), 0, ptr(mt), ptr(pos), ptr(tok[1]), B, H, N, D, dt(dtype), stream()))
    check(lib.htrvt_pool_tokens_bwd(ptr(dtok), ptr(x), ptr(keep), ptr(dx[0]), B, H, N, D, dt(dtype), stream()))
    check(lib.htrvt_pool_tokens_bwd_ps(ptr(dtok), ptr(x), ptr(keep), 0, ptr(dx[1]), B, H, N, D, dt(dtype), stream()))
    as_int = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(tok[0].view(as_int), tok[1].view(as_int)) and torch.equal(dx[0].view(as_int), dx[1].view(as_int))
    assert torch.isfinite(tok[0].float()).all() and dx[0].count_nonzero() > 0
    # a stride that is neither 0 nor N is refused, not read
    assert lib.htrvt_pool_tokens_ps(ptr(x), ptr(keep), N + 1, ptr(mt), ptr(pos), ptr(tok[1]), B, H, N, D, dt(dtype), stream()) != 0
    assert lib.htrvt_pool_tokens_bwd_ps(ptr(dtok), ptr(x), ptr(keep), 1, ptr(dx[1]), B, H, N, D, dt(dtype), stream()) != 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("form", ["bn", "bn1", "n"])
@pytest.mark.parametrize("D", [8, 64, 768])
@pytest.mark.parametrize("B,N", [(1, 1), (1, 7), (7, 1), (3, 129)])
def test_mask_tokens_matches_the_torch_expression_bitwise(B, N, D, form, dtype):
    """small-integer data: every product and sum (at most 387 rows of |dy| <= 2) is exact in float32 and bfloat16, so the
    operator must equal x * keep + (1 - keep) * mask_token and its autograd gradients bit for bit"""
    from htrvt_amd import variants
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + D)
    x = torch.randint(-4, 5, (B, N, D), generator=g).float()
    token = torch.randint(-3, 4, (1, 1, D), generator=g).float()
    dy = torch.randint(-2, 3, (B, N, D), generator=g).float()
    keep = (torch.rand((N,) if form == "n" else (B, N), generator=g) > 0.4).float()
    if form != "n" and B > 1:          # token 0: masked in sample 0 only
        keep[0, 0], keep[1:, 0] = 0.0, 1.0
    if form == "n" and N > 1:
        keep[0], keep[1] = 0.0, 1.0
    if form == "bn1":
        keep = keep.unsqueeze(-1)
    kb = keep.view(1, N, 1) if form == "n" else keep.view(B, N, 1)

    xr, tr = x.clone().requires_grad_(True), token.clone().requires_grad_(True)
    want = xr * kb + (1 - kb) * tr
    want.backward(dy)

    outs = []
    for _ in range(2):
        xd = x.to(dtype).cuda().requires_grad_(True)
        td = token.cuda().requires_grad_(True)
        y = variants.mask_tokens(xd, keep.cuda(), td)
        assert y.dtype == dtype and y.shape == (B, N, D)
        y.backward(dy.to(dtype).cuda())
        outs.append((y.detach(), xd.grad, td.grad))
    y, dx, dtoken = outs[0]
    assert torch.equal(y.float().cpu(), want.detach())
    assert torch.equal(dx.float().cpu(), xr.grad)
    assert dtoken.dtype == torch.float32 and dtoken.shape == token.shape and torch.equal(dtoken.cpu(), tr.grad)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


def test_mask_tokens_refuses_bad_arguments():
    from htrvt_amd import variants
    x, token = torch.zeros(2, 5, 8, device="cuda"), torch.zeros(8, device="cuda")
    for shape in ((4,), (3, 5), (2, 5, 2), (2, 4)):
        with pytest.raises(ValueError):
            variants.mask_tokens(x, torch.ones(shape, device="cuda"), token)
    with pytest.raises(ValueError):
        variants.mask_tokens(torch.zeros(2, 5, 6, device="cuda"), torch.ones(5, device="cuda"), torch.zeros(6, device="cuda"))
    with pytest.raises(RuntimeError, match="MI355X"):
        variants.mask_tokens(x.cpu(), torch.ones(5), token.cpu())


# ---- Engine / Trainer: the tiny model of the SGM tests -------------------------------------------------------------------

def _cfg():
    from oracle import htrvt_oracle as O
    return O.Config(80, (64, 512), embed_dim=64, depth=2, num_heads=2)


def _tiny_model(dtype=torch.float32):
    from oracle import htrvt_oracle as O
    from htrvt_amd.model import HTR_VT as M
    sd = O.init_state_dict(_cfg(), seed=7, randomize_affine=True)
    m = M.MaskedAutoencoderViT(80, img_size=[64, 512], patch_size=(4, 64), embed_dim=64, depth=2, num_heads=2, mlp_ratio=4,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _tiny_batch(golden_dir):
    t = np.load(os.path.join(golden_dir, "tiny_model.npz"))
    return (torch.from_numpy(t["x"]).cuda(), torch.from_numpy(t["targets"]), torch.from_numpy(t["lengths"]),
            torch.from_numpy(t["keep_mask"]))


def _run(golden_dir, keep, dtype=torch.float32):
    """a fresh tiny model, one forward + CTC + backward with `keep`: (logits, loss, gradients)"""
    import htrvt_amd
    x, tg, tl, _ = _tiny_batch(golden_dir)
    m = _tiny_model(dtype)
    y = m(x, keep_mask=keep)
    loss = htrvt_amd.ctc_loss(y, tg, tl)
    loss.backward()
    return y.detach(), loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _differing_rows(keep):
    """[4, N]: row 0 the recorded span mask, the others shifted / inverted / all kept"""
    return torch.stack([keep, torch.roll(keep, 5), 1.0 - keep, torch.ones_like(keep)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_equal_rows_are_the_shared_mask_bitwise(golden_dir, dtype):
    keep = _tiny_batch(golden_dir)[3]
    y0, l0, g0 = _run(golden_dir, keep, dtype)
    assert g0["mask_token"].abs().sum() > 0
    for form in (keep.expand(4, -1), keep.view(1, -1, 1).expand(4, -1, -1), keep.expand(4, -1).cuda()):
        y1, l1, g1 = _run(golden_dir, form, dtype)
        assert torch.equal(y0, y1) and torch.equal(l0, l1)
        assert set(g0) == set(g1)
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n


def test_engine_differing_rows_mask_each_sample_with_its_own_row(golden_dir):
    """fails where the engine reads row 0 for every image (the shared-mask kernels handed a [B, N] mask)"""
    keep = _tiny_batch(golden_dir)[3]
    rows = _differing_rows(keep)
    y0, l0, g0 = _run(golden_dir, keep)
    y1, l1, g1 = _run(golden_dir, rows)
    assert torch.equal(y0[0], y1[0])            # sample 0 has the same mask; the stem does not see the mask
    assert not torch.equal(y0[1], y1[1]) and not torch.equal(y0[2], y1[2]) and not torch.equal(y0[3], y1[3])
    assert not torch.equal(l0, l1) and not torch.equal(g0["mask_token"], g1["mask_token"])
    # behind the stem every sample is on its own: sample b equals sample b of a batch masked with row b throughout
    for b in (1, 2, 3):
        yb, _, _ = _run(golden_dir, rows[b].contiguous())
        assert torch.equal(yb[b], y1[b]), b


def test_engine_refuses_other_mask_shapes(golden_dir):
    x, _, _, keep = _tiny_batch(golden_dir)
    m = _tiny_model()
    N = keep.numel()
    for bad in (torch.ones(N + 1), torch.ones(N - 1), torch.ones(5, N), torch.ones(4, N - 1), torch.ones(4, N, 2),
                torch.ones(1, N), torch.ones(4 * N), torch.ones(N, 1)):
        with pytest.raises(ValueError):
            m(x, keep_mask=bad)
    assert torch.isfinite(m(x, keep_mask=torch.ones(4, N, 1))).all()


def _trainer():
    from htrvt_amd.trainer import Trainer
    m = _tiny_model()
    return m, Trainer(m, max_lr=1e-3, betas=(0.9, 0.99), weight_decay=0.5)


def test_trainer_passes_per_sample_masks_through(golden_dir):
    x, tg, tl, keep = _tiny_batch(golden_dir)
    tg, tl = tg.numpy(), tl.numpy()
    rows = _differing_rows(keep)

    def state(fn):
        m, tr = _trainer()
        loss = fn(tr).clone()
        torch.cuda.synchronize()
        return loss, tr.flat.flat_g.clone(), tr.flat.flat_p.clone()

    shared = state(lambda tr: tr.step(x, tg, tl, keep_mask=keep))
    same = state(lambda tr: tr.step(x, tg, tl, keep_mask=keep.expand(4, -1)))
    differ = state(lambda tr: tr.step(x, tg, tl, keep_mask=rows))
    assert all(torch.equal(a, b) for a, b in zip(shared, same))
    assert not torch.equal(shared[0], differ[0]) and not torch.equal(shared[1], differ[1])
    # forward_backward and both passes of sam_step
    fb = state(lambda tr: tr.forward_backward(x, tg, tl, keep_mask=rows))
    assert torch.equal(fb[0], differ[0]) and torch.equal(fb[1], differ[1])
    sam_shared = state(lambda tr: tr.sam_step(x, tg, tl, keep_mask=keep, keep_mask2=keep))
    sam_same = state(lambda tr: tr.sam_step(x, tg, tl, keep_mask=keep.expand(4, -1), keep_mask2=keep.view(1, -1, 1).expand(4, -1, -1)))
    sam_second = state(lambda tr: tr.sam_step(x, tg, tl, keep_mask=keep, keep_mask2=rows))
    assert all(torch.equal(a, b) for a, b in zip(sam_shared, sam_same))
    assert torch.equal(sam_shared[0], sam_second[0]) and not torch.equal(sam_shared[1], sam_second[1])
    with pytest.raises(ValueError):
        _trainer()[1].step(x, tg, tl, keep_mask=torch.ones(3, keep.numel()))


def test_graphed_step_refuses_a_per_sample_mask(golden_dir):
    x, tg, tl, keep = _tiny_batch(golden_dir)
    tg, tl = tg.numpy(), tl.numpy()
    m, tr = _trainer()
    tr.step(x, tg, tl, keep_mask=keep)
    gs = tr.capture_step(x, max_target_len=64, masked=True)
    before = tr.flat.flat_p.clone()
    for bad in (keep.expand(4, -1), keep.expand(4, -1).cuda(), keep.view(1, -1, 1).expand(4, -1, -1)):
        with pytest.raises(ValueError, match="per-sample"):
            gs.step(x, tg, tl, keep_mask=bad)
    torch.cuda.synchronize()
    assert torch.equal(before, tr.flat.flat_p)          # nothing ran
    assert torch.isfinite(gs.step(x, tg, tl, keep_mask=keep)).all()
