#!/usr/bin/env python3
"""Generate tests/golden/conformer_dropout.npz by running the REFERENCE FeedForward, ConvModule, ConformerBlock
(model_sgm_mms_conv/model/HTR_VT.py), SqueezeConformerBlock and SqueezeFormerEncoder
(model_sgm_mms_conv_squeeze/model/HTR_VT.py) on the CPU in float64, in TRAIN mode with non-zero rates, and recording every
mask they draw.  Runs only where the reference is checked out; the fixture holds data only.

The masks: a forward hook on each nn.Dropout reads keep = (output != 0), after asserting that the input has no exact zero;
timm is not installed, and the stand-in of tools/make_goldens.py asserts p == 0, so DropPath here restates timm's documented
rule (drop_path(x, p, training, scale_by_keep=True): one Bernoulli(1 - p) per sample, shaped [B, 1, ...], the kept samples
divided by 1 - p) and records its draw.

Stored per case of tests/conformer_dropout_refs.CASES (modules rebuilt from their seed as in squeezeformer_cases):
  {case}.sdsum          per-key float64 sums of the state_dict
  {case}.E / .S / .A    np.packbits of the element masks [blocks][4][B*N][D], the sample masks [blocks][4][B] and the
                        attention masks [blocks][B][heads][N][N] (ffn: E [B*N][D]; conv: E and S [B]); a site whose rate is 0
                        holds ones.  The encoder's second stage has N // 2 tokens: its masks are stored as .E1 / .A1
  {case}.y              the train-mode output, float64, in full (the two blocks); {case}.y.gv its probe product (every case)
  {case}.dx.gv, {case}.grad.{name}[.gv]   backward of sum(y * dy): squeezeformer_cases.probe products (tensors up to
                        PROBE_ABOVE elements in full)
    python tools/make_goldens_conformer_dropout.py
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "conformer_dropout.npz")
REFS = {"conv": "/root/reference/model_sgm_mms_conv", "squeeze": "/root/reference/model_sgm_mms_conv_squeeze"}
DRAW_SEED = 2024
FULL_Y = ("cblock", "sblock")      # the two blocks' outputs element by element; the other cases as probes, to stay small


class DropPath(nn.Module):
    """timm's rule, restated; `drawn` keeps the last keep mask [B]"""

    def __init__(self, drop_prob=0.0, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep, self.drawn = drop_prob, scale_by_keep, None

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep_prob = 1.0 - self.drop_prob
        t = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep_prob)
        self.drawn = t.reshape(-1).clone()
        if keep_prob > 0.0 and self.scale_by_keep:
            t = t.div(keep_prob)
        return x * t


def _load(which):
    import importlib.util
    ref = REFS[which]
    sys.path.insert(0, ref)
    try:
        spec = importlib.util.spec_from_file_location("ref_" + which, os.path.join(ref, "model/HTR_VT.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path.remove(ref)
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]


def _record(m):
    """hooks on every nn.Dropout of m -> {module name: keep mask}, filled by the next forward"""
    got = {}

    def hook(name):
        def fn(mod, inp, out):
            if mod.training and mod.p > 0:
                assert bool((inp[0] != 0).all()), name + ": an exact zero in a dropout input hides its mask"
                got[name] = (out != 0).double()
        return fn
    for name, mod in m.named_modules():
        if isinstance(mod, nn.Dropout):
            mod.register_forward_hook(hook(name))
    return got


def _block_masks(got, m, prefix, Bm, Nm, Dm, heads):
    """E [4][B*N][D], S [4][B], A [B][h][N][N] of the block m (module names under prefix); ones where nothing was drawn"""
    def e(name):
        t = got.get(prefix + name)
        return t.reshape(Bm * Nm, Dm) if t is not None else torch.ones(Bm * Nm, Dm, dtype=torch.float64)

    def s(site):
        dp = getattr(m, "drop_path_" + site)
        return dp.drawn.double() if isinstance(dp, DropPath) and dp.drawn is not None else torch.ones(Bm, dtype=torch.float64)
    # the conv module's dropout acts on [B, D, N]: back to token rows
    conv = got.get(prefix + "conv_module.dropout")
    conv = conv.transpose(1, 2).reshape(Bm * Nm, Dm) if conv is not None else torch.ones(Bm * Nm, Dm, dtype=torch.float64)
    E = torch.stack([e("ffn1.dropout"), e("attn.proj_drop"), conv, e("ffn2.dropout")])
    A_ = got.get(prefix + "attn.attn_drop")
    A_ = A_ if A_ is not None else torch.ones(Bm, heads, Nm, Nm, dtype=torch.float64)
    return E, torch.stack([s(n) for n in ("ffn1", "attn", "conv", "ffn2")]), A_


def _bits(t):
    return np.packbits(t.numpy().astype(bool).reshape(-1))


def main():
    from make_goldens import _install_timm_stub
    import conformer_dropout_refs as DR
    import squeezeformer_cases as C
    _install_timm_stub()
    sys.modules["timm.models.vision_transformer"].DropPath = DropPath
    # squeezeformer_cases.build looks every constructor up in one namespace: the squeeze fork's, with the conv fork's ConformerBlock
    M = types.SimpleNamespace(**{n: getattr(_load("squeeze"), n) for n in (
        "FeedForward", "ConvModule", "SqueezeExcite1D", "Downsample1D", "Upsample1D", "SqueezeConformerBlock",
        "SqueezeFormerEncoder")}, ConformerBlock=_load("conv").ConformerBlock)
    out = {}
    for case, (kind, args, kwargs, Bm, Nm) in DR.CASES.items():
        m = DR.case_module(M, case)
        out[case + ".sdsum"] = np.array([float(v.double().sum()) for v in m.state_dict().values()])
        m = m.double().train()
        got = _record(m)
        x, dy = DR.inputs(case)
        paths = [mod for mod in m.modules() if isinstance(mod, DropPath) and mod.drop_prob > 0]
        for seed in range(DRAW_SEED, DRAW_SEED + 100):    # the first seed at which every drop-path site keeps and drops a sample
            got.clear()
            xr = x.double().requires_grad_(True)
            torch.manual_seed(seed)
            y = m(xr)
            if all(0 < float(mod.drawn.sum()) < Bm for mod in paths):
                break
        else:
            raise RuntimeError(case + ": no seed with mixed drop-path draws")
        out[case + ".seed"] = np.array(seed)
        (y * dy.double()).sum().backward()
        Dm = args[0]
        if kind == "ffn":
            out[case + ".E"] = _bits(got["dropout"].reshape(Bm * Nm, Dm))
        elif kind == "conv":
            out[case + ".E"] = _bits(got["dropout"].transpose(1, 2).reshape(Bm * Nm, Dm))
            out[case + ".S"] = _bits(m.drop_path.drawn)
            assert 0 < float(m.drop_path.drawn.sum()) < Bm
        elif kind in ("cblock", "sblock"):
            E, S_, A_ = _block_masks(got, m, "", Bm, Nm, Dm, args[1])
            out[case + ".E"], out[case + ".S"], out[case + ".A"] = _bits(E[None]), _bits(S_[None]), _bits(A_[None])
            assert all(0 < float(s.sum()) < Bm for s in S_), "a drop-path site kept or dropped every sample: another DRAW_SEED"
        else:
            assert len(m.stage1) == 1 and len(m.stage2) == 1
            E0, S0, A0 = _block_masks(got, m.stage1[0], "stage1.0.", Bm, Nm, Dm, args[1])
            E1, S1, A1 = _block_masks(got, m.stage2[0], "stage2.0.", Bm, Nm // 2, Dm, args[1])
            out[case + ".E"], out[case + ".E1"] = _bits(E0), _bits(E1)
            out[case + ".S"] = _bits(torch.stack([S0, S1]))
            out[case + ".A"], out[case + ".A1"] = _bits(A0), _bits(A1)
            assert all(0 < float(s.sum()) < Bm for s in S1)
        if kind in FULL_Y:
            out[case + ".y"] = y.detach().double().numpy()
        out[case + ".y.gv"] = C.probe(y, True).numpy()
        out[case + ".dx.gv"] = C.probe(xr.grad, True).numpy()
        for n, p in m.named_parameters():
            if p.numel() > C.PROBE_ABOVE:
                out[f"{case}.grad.{n}.gv"] = C.probe(p.grad).numpy()
            else:
                out[f"{case}.grad.{n}"] = p.grad.detach().double().numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
