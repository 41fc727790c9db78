#!/usr/bin/env python3
"""Generate tests/golden/sgm_mms.npz by running the REFERENCE multi-mask SGM fork (model_sgm_mms_attach/model/HTR_VT.py,
the same file as model_sgm_mms_detach's) on the CPU, with the in-memory timm stand-in of tools/make_goldens.py.  Runs only
where the reference tree is checked out (its root: $HTRVT_REFERENCE, default /root/reference); the fixture holds data
only.  Inputs and weights are rebuilt from seeds on both sides (tests/sgm_mms_cases.py).  Stored:
  gen.{case}.*    the fork's mask generators after random.seed(s); torch.manual_seed(s) (sgm_mms_cases.GEN_CASES): the
                  mask bool [B, L] (True = masked), the next random.random() and torch.rand(1) behind the call, and the
                  loop trials the call needed (random.randint calls / 2).  A case that reaches the fork's cap of 10 000
                  trials in a sample is refused here.
  init.*          create_model(80, (64, 512)) after manual_seed(123): state_dict keys, shapes, per-key sums
  model.eval      eval logits of the tiny model (sgm_mms_cases.model_*), float32 like everything below
  model.{mode}.*  one train-mode pass per mask mode with seeded generators: the mask, logits (every second token), features
                  (every fourth), CTC loss, the gradients of ctc + FEAT_WEIGHT mean(feats^2) (whole up to FULL_GRAD
                  elements, else a fixed sample of GRAD_SAMPLE entries + the norm) and the BatchNorm buffers behind the pass
  tri.*           one tri_masked_loss-shaped step (train.py:76-97): random, block, span_old passes on one model, the
                  gradients of the mean of the three losses and the BatchNorm buffers after the three updates
    python tools/make_goldens_sgm_mms.py
"""
import importlib.util
import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "sgm_mms.npz")
REF = os.path.join(os.environ.get("HTRVT_REFERENCE", "/root/reference"), "model_sgm_mms_attach")
CAP = 10000


def _load():
    sys.path.insert(0, REF)
    try:
        spec = importlib.util.spec_from_file_location("ref_sgm_mms_model", os.path.join(REF, "model", "HTR_VT.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]


class _CountRandint:
    """counts the fork's random.randint calls (two per loop trial) without touching the stream"""

    def __enter__(self):
        self.calls, self._orig = 0, random.randint

        def counted(a, b):
            self.calls += 1
            return self._orig(a, b)
        random.randint = counted
        return self

    def __exit__(self, *exc):
        random.randint = self._orig


def _grads(out, pre, model):
    import sgm_mms_cases as C
    for n, p in model.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().numpy().ravel()
        if g.size <= C.FULL_GRAD:
            out[f"{pre}grad.{n}"] = g.astype(np.float32)
        else:
            out[f"{pre}gsample.{n}"] = g[C.sample_index(g.size)].astype(np.float32)
            out[f"{pre}gnorm.{n}"] = np.float64(np.linalg.norm(g))


def _buffers(out, pre, model):
    for n, b in model.named_buffers():
        if "running" in n:
            out[f"{pre}buf.{n}"] = b.numpy().astype(np.float32)


def main():
    from functools import partial
    from make_goldens import _install_timm_stub
    import sgm_mms_cases as C
    _install_timm_stub()
    ref = _load()
    torch.set_num_threads(8)
    out = {}

    # ---- the generators ----
    gm = ref.MaskedAutoencoderViT(80, img_size=[64, 64], patch_size=(4, 64), embed_dim=8, depth=1, num_heads=1, mlp_ratio=1,
                                  norm_layer=partial(nn.LayerNorm, eps=1e-6))
    capped = []
    for i, (name, kind, B, L, kw) in enumerate(C.GEN_CASES):
        kw = dict(kw)
        random.seed(C.gen_seed(i))
        torch.manual_seed(C.gen_seed(i))
        with _CountRandint() as cnt:
            if kind == "random":
                mask = gm._mask_random_1d(B, L, kw["ratio"], "cpu")
            elif kind == "block":
                mask = gm._mask_block_1d(B, L, kw["ratio"], "cpu", **({"min_block": kw["min_block"]} if "min_block" in kw else {}))
            elif kind == "span":
                mask = gm._mask_span_1d(B, L, kw["ratio"], kw["max_span"], "cpu")
            elif kind == "span_old":
                mask = gm._mask_span_old_1d(B, L, kw["ratio"], kw["max_span"], "cpu")
            else:
                ratios = kw.pop("mms_ratios", None)
                if ratios is not None:
                    gm.mms_ratios = ratios
                keep = gm.generate_mms_mask(torch.zeros(B, L, 1), **kw)
                if ratios is not None:
                    del gm.mms_ratios
                assert keep.shape == (B, L, 1) and keep.dtype == torch.float32
                mask = keep[..., 0] == 0
        trials = cnt.calls // 2
        # fewer than CAP trials in the whole call: no sample's loop can have run into the cap
        if trials >= CAP:
            capped.append((name, trials))
        assert mask.shape == (B, L) and mask.dtype == torch.bool
        out[f"gen.{name}.mask"] = mask.numpy()
        out[f"gen.{name}.next_random"] = np.float64(random.random())
        out[f"gen.{name}.next_torch"] = torch.rand(1).numpy()
        out[f"gen.{name}.trials"] = np.int64(trials)
    assert not capped, f"the fork's loops may have hit their cap in {capped}: take these cases out of GEN_CASES"
    print(len(C.GEN_CASES), "generator cases, most trials:", max(int(out[k]) for k in out if k.endswith(".trials")))

    # ---- construction ----
    torch.manual_seed(123)
    sd = ref.create_model(80, (64, 512)).state_dict()
    out["init.keys"] = np.array(list(sd.keys()))
    out["init.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["init.sums"] = np.array([float(v.double().sum()) for v in sd.values()])

    # ---- the tiny model, in float32 as the fork trains it.  (Its float64 run is NOT the yardstick here: float32 max-pool
    # windows and ReLU inputs tie or change sides where float64 separates them, and the fork's own float32 run is then up to
    # 1.9e-2 of the max-abs away from its float64 run on stem gradients -- patch_embed.layer2.0.bn1.bias, block mode.) ----
    def tiny():
        m = ref.MaskedAutoencoderViT(80, img_size=[64, 512], patch_size=(4, 64), embed_dim=64, depth=2, num_heads=2, mlp_ratio=4,
                                     norm_layer=partial(nn.LayerNorm, eps=1e-6))
        m.load_state_dict(C.model_state_dict(), strict=True)
        return m

    x, tg, ln = C.model_batch(os.path.join(ROOT, "tests", "golden"))
    crit = nn.CTCLoss(reduction="none", zero_infinity=True)

    def one_pass(m, mode):
        """the fork's compute_losses shape: (loss, ctc, logits, feats, the mask of the pass)"""
        seen = []
        for attr in ("_mask_random_1d", "_mask_block_1d", "_mask_span_old_1d"):
            orig = getattr(type(m), attr)
            setattr(m, attr, lambda *a, _o=orig, **k: seen.append(_o(m, *a, **k)) or seen[-1])
        orig_mms = type(m).generate_mms_mask
        m.generate_mms_mask = lambda *a, **k: seen.append(orig_mms(m, *a, **k)) or seen[-1]
        logits, feats = m(x, **C.mode_kwargs(mode))
        mask = seen[-1]
        mask = (mask[..., 0] == 0) if mask.dtype != torch.bool else mask
        lp = logits.permute(1, 0, 2).log_softmax(2)
        ctc = crit(lp, tg.long(), torch.full((x.shape[0],), logits.shape[1], dtype=torch.int32), ln.long()).mean()
        return ctc + C.FEAT_WEIGHT * feats.square().mean(), ctc, logits, feats, mask

    m = tiny().eval()
    with torch.no_grad():
        out["model.eval"] = m(x).numpy().astype(np.float32)
    for mode in C.MODES:
        m = tiny().train()
        random.seed(C.mode_seed(mode))
        torch.manual_seed(C.mode_seed(mode))
        loss, ctc, logits, feats, mask = one_pass(m, mode)
        loss.backward()
        pre = f"model.{mode}."
        out[pre + "mask"] = mask.numpy()
        out[pre + "logits"] = logits.detach()[:, C.LOGIT_TOKENS].numpy().astype(np.float32)
        out[pre + "feats"] = feats.detach()[:, C.FEAT_TOKENS].numpy().astype(np.float32)
        out[pre + "ctc"] = np.float64(ctc.item())
        out[pre + "loss"] = np.float64(loss.item())
        _grads(out, pre, m)
        _buffers(out, pre, m)
        print(f"{mode}: masked {mask.float().mean(1).tolist()}, ctc {ctc.item():.6f}, loss {loss.item():.6f}")

    m = tiny().train()
    random.seed(C.TRI_SEED)
    torch.manual_seed(C.TRI_SEED)
    total = 0.0
    for j, mode in enumerate(C.TRI_MODES):
        loss, ctc, _, _, mask = one_pass(m, mode)
        total = total + loss
        out[f"tri.mask.{mode}"] = mask.numpy()
        out[f"tri.ctc.{mode}"] = np.float64(ctc.item())
    (total / len(C.TRI_MODES)).backward()
    out["tri.loss"] = np.float64(total.item() / len(C.TRI_MODES))
    _grads(out, "tri.", m)
    _buffers(out, "tri.", m)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
