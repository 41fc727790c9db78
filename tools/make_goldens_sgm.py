#!/usr/bin/env python3
"""Generate tests/golden/sgm.npz by running the REFERENCE SGM head (model_sgm_2/model/sgm_head.py, byte-identical in all
eleven SGM forks) and model_sgm_2's encoder on the CPU in float64, with the timm stand-in of tools/make_goldens.py.  Runs
only where the reference is checked out; the fixture holds data only.  Inputs are rebuilt from seeds on both sides
(tests/sgm_cases.py).  Stored:
  init.*          SGMHead(768, 84) after manual_seed(123): state_dict keys, shapes, per-key sums
  vocab.itos      build_sgm_vocab of an 80-class converter
  ctx.* / ctx0.*  make_context_batch of tests/sgm_cases.CONTEXT_TEXTS (edge cases) / of two empty lines (Lmax = 0)
  head.{case}.*   eval-mode head forward + backward of sgm_cases.HEAD_CASES: the context batch, loss, logits, every parameter
                  gradient and d vis_tokens (small: whole tensors; d768: sums, norms and a fixed sample of 1024 entries)
  model.*         the tiny model of tiny_model.npz with return_features=True (train mode, its recorded span mask): the
                  features, ctc + 1.0 * sgm and the gradients of a handful of encoder and stem tensors
    python tools/make_goldens_sgm.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "sgm.npz")
REF = "/root/reference/model_sgm_2"
MODEL_GRADS = ("norm.weight", "norm.bias", "head.weight", "blocks.1.mlp.fc2.weight", "blocks.0.attn.qkv.weight",
               "mask_token", "patch_embed.layer3.1.conv2.weight", "patch_embed.conv1.weight")
SAMPLE = 1024


def _load(name, rel):
    sys.path.insert(0, REF)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]


def sample_idx(n, key):
    return np.sort(np.random.default_rng(key).choice(n, size=min(n, SAMPLE), replace=False))


def main():
    from make_goldens import _install_timm_stub
    import sgm_cases as C
    _install_timm_stub()
    H = _load("ref_sgm_head", "model/sgm_head.py")
    M = _load("ref_sgm_model", "model/HTR_VT.py")
    torch.set_num_threads(8)
    out = {}

    torch.manual_seed(123)
    sd = H.SGMHead(768, 84).state_dict()
    out["init.keys"] = np.array(list(sd.keys()))
    out["init.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["init.sums"] = np.array([float(v.double().sum()) for v in sd.values()])

    stoi, itos, *_ = H.build_sgm_vocab(C.Converter())
    out["vocab.itos"] = np.array(itos)
    for key, texts in (("ctx", C.CONTEXT_TEXTS), ("ctx0", ["", ""])):
        for n, t in zip(("left", "right", "tgt", "mask"), H.make_context_batch(texts, stoi, 5, device="cpu")):
            out[f"{key}.{n}"] = t.numpy()

    for case, (B, L, N, D, dtx, V, S) in C.HEAD_CASES.items():
        seed, texts, vis = C.head_inputs(case)
        stoi_v = C.vocab_for(V)
        ctx = H.make_context_batch(texts, stoi_v, S, device="cpu")
        torch.manual_seed(seed)
        head = H.SGMHead(D, V, d_txt=dtx, sub_str_len=S)
        C.perturb_head(head, seed)
        head = head.double().eval()
        v64 = vis.double().requires_grad_(True)
        res = head(v64, *ctx)
        res["loss_sgm"].backward()
        pre = f"head.{case}."
        for n, t in zip(("left", "right", "tgt", "mask"), ctx):
            out[pre + n] = t.numpy()
        out[pre + "loss"] = np.float64(res["loss_sgm"].item())
        out[pre + "logits_l"] = res["logits_l"].detach().numpy()
        out[pre + "logits_r"] = res["logits_r"].detach().numpy()
        grads = {n: p.grad for n, p in head.named_parameters()}
        grads["vis"] = v64.grad
        for n, gr in grads.items():
            a = gr.numpy().reshape(-1)
            if case == "small":
                out[pre + "grad." + n] = gr.numpy()
            else:
                idx = sample_idx(a.size, len(n) * 7919 + a.size)
                out[pre + "gsum." + n] = np.float64(a.sum())
                out[pre + "gnorm." + n] = np.float64(np.linalg.norm(a))
                out[pre + "gmax." + n] = np.float64(np.abs(a).max())
                out[pre + "gidx." + n] = idx
                out[pre + "gval." + n] = a[idx]

    # ---- the tiny model (tiny_model.npz) with the feature tap, ctc + 1.0 * sgm ----
    from functools import partial
    from oracle import htrvt_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "tiny_model.npz"))
    cfg = O.Config(80, (64, 512), embed_dim=64, depth=2, num_heads=2)
    sdm = O.init_state_dict(cfg, seed=7, randomize_affine=True)
    m = M.MaskedAutoencoderViT(80, img_size=[64, 512], patch_size=(4, 64), embed_dim=64, depth=2, num_heads=2, mlp_ratio=4,
                               norm_layer=partial(nn.LayerNorm, eps=1e-6))
    m.load_state_dict(sdm, strict=True)
    m = m.double().train()
    x = torch.from_numpy(g["x"]).double()
    torch.manual_seed(11)                        # the span mask of tiny_model.npz (keep_mask)
    logits, feats = m(x, 0.4, 8, use_masking=True, return_features=True)
    lp = logits.permute(1, 0, 2).log_softmax(2)
    crit = torch.nn.CTCLoss(reduction="none", zero_infinity=True)
    ctc = crit(lp, torch.from_numpy(g["targets"]).long(), torch.IntTensor([lp.shape[0]] * 4),
               torch.from_numpy(g["lengths"]).long()).mean()
    texts = C.random_texts(4, 30, 84, seed=4)
    ctx = H.make_context_batch(texts, C.vocab_for(84), 5, device="cpu")
    torch.manual_seed(77)
    head = H.SGMHead(64, 84, d_txt=32)
    C.perturb_head(head, 77)
    head = head.double().eval()
    sgm = head(feats, *ctx)["loss_sgm"]
    total = ctc + 1.0 * sgm
    total.backward()
    out["model.feats"] = feats.detach().float().numpy()
    out["model.logits"] = logits.detach().float().numpy()
    out["model.ctc"] = np.float64(ctc.item())
    out["model.sgm"] = np.float64(sgm.item())
    params = dict(m.named_parameters())
    for n in MODEL_GRADS:
        out["model.grad." + n] = params[n].grad.numpy()
    for k in list(out):
        if out[k].dtype == np.float64 and out[k].ndim > 0:
            out[k] = out[k].astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
