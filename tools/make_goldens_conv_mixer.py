#!/usr/bin/env python3
"""Generate tests/golden/conv_mixer.npz by running the REFERENCE ConvLocalMixer1D (model_sgm_macaron/model/HTR_VT.py; the
copy in model_sgm_macaron_2 is identical) on the CPU in float64, with the timm stand-in of tools/make_goldens.py.  Runs
only where the reference is checked out; the fixture holds data only.  Stored:
  init.{bn,nobn}.*   ConvLocalMixer1D(64, 7, use_bn=...) after manual_seed(123): state_dict keys, shapes, per-key sums
  sd.*               the perturbed state_dict (tests/conv_mixer_cases.perturb of the seed-123 module with BatchNorm), float32:
                     the module of every case; the use_bn=False case takes its shared entries from it and adds
                     nobn.dwconv.bias
  {case}.*           x, dy (float32 inputs), y_eval, y_train (train mode, drop.p = 0), dx and grad.* (backward of
                     sum(y_train * dy)), running_mean / running_var / num_batches_tracked after the train forward (float64)
    python tools/make_goldens_conv_mixer.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "conv_mixer.npz")
REF = "/root/reference/model_sgm_macaron"


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


def main():
    from make_goldens import _install_timm_stub
    import conv_mixer_cases as C
    _install_timm_stub()
    M = _load("ref_macaron_model", "model/HTR_VT.py")
    out = {}
    for tag, use_bn in (("bn", True), ("nobn", False)):
        torch.manual_seed(C.INIT_SEED)
        sd = M.ConvLocalMixer1D(C.D, C.K, use_bn=use_bn).state_dict()
        out[f"init.{tag}.keys"] = np.array(list(sd.keys()))
        out[f"init.{tag}.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        out[f"init.{tag}.sums"] = np.array([float(v.double().sum()) for v in sd.values()])

    torch.manual_seed(C.INIT_SEED)
    base = C.perturb(M.ConvLocalMixer1D(C.D, C.K, use_bn=True)).state_dict()
    for k, v in base.items():
        out["sd." + k] = v.numpy().copy()
    bias = 0.2 * torch.randn(C.D, generator=torch.Generator().manual_seed(9))
    out["nobn.dwconv.bias"] = bias.numpy().copy()

    for case, (B, N, use_bn, _) in C.CASES.items():
        m = M.ConvLocalMixer1D(C.D, C.K, drop=0.0, use_bn=use_bn)
        sd = {k: v.clone() for k, v in base.items() if k in m.state_dict()}
        if not use_bn:
            sd["dwconv.bias"] = bias.clone()
        m.load_state_dict(sd, strict=True)
        m = m.double()
        x, dy = C.inputs(case)
        pre = case + "."
        out[pre + "x"], out[pre + "dy"] = x.numpy(), dy.numpy()
        with torch.no_grad():
            out[pre + "y_eval"] = m.eval()(x.double()).numpy()
        xr = x.double().requires_grad_(True)
        y = m.train()(xr)
        (y * dy.double()).sum().backward()
        out[pre + "y_train"] = y.detach().numpy()
        out[pre + "dx"] = xr.grad.numpy()
        for n, p in m.named_parameters():
            out[pre + "grad." + n] = p.grad.numpy()
        if use_bn:
            out[pre + "running_mean"] = m.bn.running_mean.numpy().copy()
            out[pre + "running_var"] = m.bn.running_var.numpy().copy()
            out[pre + "num_batches_tracked"] = m.bn.num_batches_tracked.numpy().copy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
