#!/usr/bin/env python3
"""Generate tests/golden/sgm_localglobal.npz by running the REFERENCE SGM local-global fork
(model_sgm_localglobal/model/HTR_VT.py) on CPU in float64.  Runs only in the dev container (needs /root/reference); the
fixture holds data only.  timm (absent here) is replaced by the in-memory Mlp / DropPath stand-in of tools/make_goldens.py.

Weights are NOT stored: both sides rebuild them -- `torch.manual_seed(123)` + construction, which the drop-in reproduces
bit for bit (tests/test_sgm_localglobal_cpu.py), then `perturb()` (shared with the tests via
tests/sgm_localglobal_cases.py).  Stored:
  tiny.{W}.*  d256 / 4 heads, B = 2, 64 x W for W in (256, 800) (N = 64: pad 8; N = 200: pad 4, the wrap-around window of
              the shifted block differs from its ragged one): eval logits and features; train logits, features and CTC
              loss with the seeded span mask; parameter gradients of loss_ctc + sum(feats * R) for the seeded R (whole
              tensors up to 4096 elements, else a fixed sample of 1024 entries + the norm); BN buffers after the step.
              Logits / features above 16384 elements: a fixed sample of 8192 entries (`.s`) + the norm (`.n`)
  d768.*      create_model(80, (64, 512)) seed 123: keys, shapes, per-key sums; eval logits of one image (N = 128)
    python tools/make_goldens_sgm_localglobal.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "sgm_localglobal.npz")
REF = "/root/reference/model_sgm_localglobal"


def _load():
    sys.path.insert(0, REF)
    try:
        spec = importlib.util.spec_from_file_location("ref_sgm_localglobal_model", os.path.join(REF, "model", "HTR_VT.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]


def main():
    from make_goldens import _install_timm_stub
    _install_timm_stub()
    import sgm_localglobal_cases as SC
    from functools import partial
    ref = _load()
    torch.set_num_threads(8)
    out = {}

    def put_act(key, t):
        a = t.detach().numpy().ravel()
        if a.size <= SC.FULL_ACT:
            out[key] = a.reshape(tuple(t.shape)).astype(np.float32)
        else:
            out[key + ".s"] = a[SC.act_index(a.size)].astype(np.float32)
            out[key + ".n"] = np.float64(np.linalg.norm(a))

    for W, patch in SC.TINY.items():
        torch.manual_seed(123)
        m = ref.MaskedAutoencoderViT(SC.NB_CLS, img_size=[64, W], patch_size=patch, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                                     **SC.TINY_KW)
        kinds = [(b.attn.win, b.attn.shift) if isinstance(b, ref.LocalBlock1D) else None for b in m.blocks]
        assert kinds == SC.KINDS, kinds
        SC.perturb(m)
        m = m.double()
        x, tg, ln = SC.tiny_batch(W)
        m.eval()
        with torch.no_grad():
            y, f = m(x.double(), return_features=True)
        put_act(f"tiny.{W}.eval", y)
        put_act(f"tiny.{W}.eval_feats", f)
        m.train()
        torch.manual_seed(SC.MASK_SEED)
        y, f = m(x.double(), SC.MASK_RATIO, SC.MAX_SPAN, use_masking=True, return_features=True)
        lp = y.permute(1, 0, 2).log_softmax(2)
        per = nn.CTCLoss(reduction="none", zero_infinity=True)(lp, tg, torch.full((x.shape[0],), y.shape[1], dtype=torch.int32), ln)
        loss = per.mean()
        R = SC.feature_weights(*f.shape).double()
        (loss + (f * R).sum()).backward()
        put_act(f"tiny.{W}.train", y)
        put_act(f"tiny.{W}.train_feats", f)
        out[f"tiny.{W}.loss"] = np.float64(loss.item())
        for n, p in m.named_parameters():
            if not p.requires_grad:         # pos_embed
                continue
            g = p.grad.detach().numpy().ravel()
            if g.size <= SC.FULL_GRAD:
                out[f"tiny.{W}.grad.{n}"] = g.astype(np.float32)
            else:
                out[f"tiny.{W}.gsample.{n}"] = g[SC.sample_index(g.size)].astype(np.float32)
                out[f"tiny.{W}.gnorm.{n}"] = np.float64(np.linalg.norm(g))
        for n, b in m.named_buffers():
            if "running" in n:
                out[f"tiny.{W}.buf.{n}"] = b.numpy().astype(np.float32)
        print(f"tiny {W}: N = {y.shape[1]}, loss {loss.item():.6f}, feature term {(f * R).sum().item():.6f}")

    torch.manual_seed(123)
    m = ref.create_model(80, (64, 512))
    sd = m.state_dict()
    out["d768.keys"] = np.array(list(sd.keys()))
    out["d768.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["d768.sums"] = np.array([float(v.double().sum()) for v in sd.values()])
    m = m.double().eval()
    with torch.no_grad():
        out["d768.eval"] = m(SC.d768_images().double()).numpy().astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
