#!/usr/bin/env python3
"""Generate tests/golden/squeezeformer.npz by running the REFERENCE FeedForward, ConvModule, ConformerBlock, SqueezeExcite1D,
Downsample1D, Upsample1D, SqueezeConformerBlock and SqueezeFormerEncoder (model_sgm_mms_conv_squeeze/model/HTR_VT.py; lines
1-168 of model_sgm_mms_conv/model/HTR_VT.py are identical) on the CPU in float64, with the timm stand-in of
tools/make_goldens.py.  Runs only where the reference is checked out; the fixture holds data only.
Stored (tests/squeezeformer_cases.py defines the modules, cases, inputs and probes):
  init.{kind}.keys / .shapes / .sums   each module of INIT after manual_seed(123): state_dict keys, shapes, per-key sums
  {case}.sdsum      per-key float64 sums of the case's state_dict (the module is rebuilt from its seed by case_module)
  {case}.y, .dx, .grad.{name}   train forward, backward of sum(y * dy) -- in full up to PROBE_ABOVE elements, else as
                    .gv, the product with the seeded probe vector
    python tools/make_goldens_squeezeformer.py
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
OUT = os.path.join(ROOT, "tests", "golden", "squeezeformer.npz")
REF = "/root/reference/model_sgm_mms_conv_squeeze"


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


def _store(out, key, t, C, activation=False):
    if t.numel() > C.PROBE_ABOVE:
        out[key + ".gv"] = C.probe(t, activation).numpy()
    else:
        out[key] = t.detach().double().numpy()


def main():
    from make_goldens import _install_timm_stub
    import squeezeformer_cases as C
    _install_timm_stub()
    M = _load("ref_squeezeformer_model", "model/HTR_VT.py")
    out = {}
    for tag, (kind, args, kwargs) in C.INIT.items():
        torch.manual_seed(C.INIT_SEED)
        sd = C.build(M, kind, args, kwargs).state_dict()
        out[f"init.{tag}.keys"] = np.array(list(sd.keys()))
        out[f"init.{tag}.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        out[f"init.{tag}.sums"] = np.array([float(v.double().sum()) for v in sd.values()])
    for case, (kind, _, _, _, _) in C.CASES.items():
        m = C.case_module(M, case)
        sd = m.state_dict()
        out[case + ".sdsum"] = np.array([float(v.double().sum()) for v in sd.values()])
        m = m.double().train()
        x, dy = C.inputs(case)
        xr = x.double().requires_grad_(True)
        y = m(xr, C.UP_TARGET[case]) if kind == "up" else m(xr)
        (y * dy.double()).sum().backward()
        _store(out, case + ".y", y, C, True)
        _store(out, case + ".dx", xr.grad, C, True)
        for n, p in m.named_parameters():
            _store(out, f"{case}.grad.{n}", p.grad, C)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
