#!/usr/bin/env python3
"""Generate tests/golden/lgp_model.npz by running the REFERENCE LGP fork (model_lgp/model/HTR_VT.py + plg.py) on CPU in
float64.  Runs only in the dev container (needs /root/reference); the fixture holds data only.  timm (absent here) is
replaced by the in-memory Mlp / DropPath stand-in of tools/make_goldens.py, also under the `timm.models.layers` name
plg.py imports.

Weights are NOT stored: both sides rebuild them -- `torch.manual_seed(123)` + construction, which the drop-in reproduces
bit for bit (tests/test_lgp_model_cpu.py), then `perturb()` (shared with the tests via tests/lgp_cases.py).  Stored:
  tiny.{W}.*  d256 / 4 blocks / 4 heads, B = 2, 64 x W for W in (256, 800) (N = 64: pad 8, G = N; N = 200: pad 4, 64 uneven
              overlapping bins): eval logits, train logits + CTC loss with the seeded span mask, parameter gradients (whole
              tensors up to 4096 elements, else a fixed sample of 1024 entries + the norm), BN buffers after the train step
  d768.*      create_model(80, (64, 512)) seed 123: keys, shapes, per-key sums; eval logits of one image (N = 128)
    python tools/make_goldens_lgp.py
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
OUT = os.path.join(ROOT, "tests", "golden", "lgp_model.npz")
REF = "/root/reference/model_lgp"


def _install_stub():
    import types
    from make_goldens import _install_timm_stub
    _install_timm_stub()
    vt = sys.modules["timm.models.vision_transformer"]
    layers = types.ModuleType("timm.models.layers")
    layers.Mlp, layers.DropPath = vt.Mlp, vt.DropPath
    sys.modules["timm.models"].layers = layers
    sys.modules["timm.models.layers"] = layers


def _load():
    sys.path.insert(0, REF)
    try:
        spec = importlib.util.spec_from_file_location("ref_lgp_model", os.path.join(REF, "model", "HTR_VT.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]


def main():
    _install_stub()
    import lgp_cases as LC
    from functools import partial
    ref = _load()
    torch.set_num_threads(8)
    out = {}
    for W in LC.TINY_WIDTHS:
        torch.manual_seed(123)
        m = ref.MaskedAutoencoderViT(LC.NB_CLS, img_size=[64, W], patch_size=(4, 64), embed_dim=256, depth=4, num_heads=4,
                                     mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6))
        LC.perturb(m)
        m = m.double()
        x, tg, ln = LC.tiny_batch(W)
        m.eval()
        with torch.no_grad():
            m(x.double())
        m.pos_embed = m.pos_embed.double()      # built lazily by the first forward, in float32
        with torch.no_grad():
            out[f"tiny.{W}.eval"] = m(x.double()).numpy().astype(np.float32)
        m.train()
        torch.manual_seed(LC.MASK_SEED)
        y = m(x.double(), LC.MASK_RATIO, LC.MAX_SPAN, use_masking=True)
        lp = y.permute(1, 0, 2).log_softmax(2)
        per = nn.CTCLoss(reduction="none", zero_infinity=True)(lp, tg, torch.full((x.shape[0],), y.shape[1], dtype=torch.int32), ln)
        loss = per.mean()
        loss.backward()
        out[f"tiny.{W}.train"] = y.detach().numpy().astype(np.float32)
        out[f"tiny.{W}.loss"] = np.float64(loss.item())
        for n, p in m.named_parameters():
            g = p.grad.detach().numpy().ravel()
            if g.size <= LC.FULL_GRAD:
                out[f"tiny.{W}.grad.{n}"] = g.astype(np.float32)
            else:
                out[f"tiny.{W}.gsample.{n}"] = g[LC.sample_index(g.size)].astype(np.float32)
                out[f"tiny.{W}.gnorm.{n}"] = np.float64(np.linalg.norm(g))
        for n, b in m.named_buffers():
            if "running" in n:
                out[f"tiny.{W}.buf.{n}"] = b.numpy().astype(np.float32)
        print(f"tiny {W}: N = {y.shape[1]}, loss {loss.item():.6f}")

    torch.manual_seed(123)
    m = ref.create_model(80, (64, 512))
    sd = m.state_dict()
    out["d768.keys"] = np.array(list(sd.keys()))
    out["d768.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["d768.sums"] = np.array([float(v.double().sum()) for v in sd.values()])
    m = m.double().eval()
    x = LC.d768_images()
    with torch.no_grad():
        m(x.double())
        m.pos_embed = m.pos_embed.double()
        out["d768.eval"] = m(x.double()).numpy().astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
