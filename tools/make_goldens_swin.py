#!/usr/bin/env python3
"""Generate tests/golden/swin.npz by running the REFERENCE WindowAttention2D, SwinBlock2D, HeightOnlyPatchMerging and
Combining (model_sgm_mms_swin/model/HTR_VT.py, torch only) on the CPU in float64.  Runs only where the reference is checked
out; the fixture holds data only.
Stored:
  init.{attn,block,merge,comb}.*  the four modules of swin_cases.INIT, each after manual_seed(123): state_dict keys, shapes,
                        per-key sums
  sd.{attn,block,merge,comb}.*    their perturbed state_dicts (swin_cases.perturb), as stored: float32, the index int64
  {case}.x, .dy         the float32 inputs of swin_cases.inputs
  {case}.sums.{tag}.*   float64 sum of every state_dict entry of the case's modules (swin_cases.case_modules rebuilds them
                        from their seeds; the sums tell a rebuilt module from the one that ran here)
  {case}.y, .dx         the output and the input gradient of sum(y * dy), float64
  {case}.grad.{tag}.*   every parameter gradient; one of more than swin_cases.PROBE_ABOVE elements as .gv / .ug / .max
                        (swin_cases.probe)
Limitation: a case's modules are not in the fixture (two million parameters against 1 MB).  The tests rebuild them from
torch's CPU sampling streams (kaiming_uniform_, trunc_normal_, randn) and recognise them by the stored per-entry sums within
swin_cases.SUM_TOL per element -- 0.2 on the sum of a 196k-element weight, enough to tell a wrong seed (0.1 per element) but no
more.  A torch release that changes those streams fails every module test with no change here: regenerate the fixture with
this script under that torch, and check that tests/test_swin_cpu.py still reproduces it to 1e-10.
    python tools/make_goldens_swin.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "swin.npz")
REF = "/root/reference/model_sgm_mms_swin"


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
    import swin_cases as C
    M = _load("ref_swin_model", "model/HTR_VT.py")
    out = {}
    for tag, (kind, args, kwargs) in C.INIT.items():
        torch.manual_seed(C.INIT_SEED)
        sd = C.build(M, kind, args, kwargs).state_dict()
        out[f"init.{tag}.keys"] = np.array(list(sd.keys()))
        out[f"init.{tag}.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        out[f"init.{tag}.sums"] = np.array([float(v.double().sum()) for v in sd.values()])
        torch.manual_seed(C.INIT_SEED)
        for k, v in C.perturb(C.build(M, kind, args, kwargs)).state_dict().items():
            out[f"sd.{tag}.{k}"] = v.numpy().copy()

    for case, (B, H, W, _, _) in C.CASES.items():
        x, dy = C.inputs(case)
        out[f"{case}.x"], out[f"{case}.dy"] = x.numpy(), dy.numpy()
        mods = C.case_modules(M, case)
        for tag, _, _, m in mods:
            for k, v in m.state_dict().items():
                out[f"{case}.sums.{tag}.{k}"] = np.array(float(v.double().sum()))
            m.double().train()
        xr = x.double().requires_grad_(True)
        t, h, w = xr, H, W
        for _, kind, _, m in mods:
            if kind == "merge":
                t, h, w = m(t, h, w)
            else:
                t = m(t, h, w)
                h = 1 if kind == "comb" else h
        (t * dy.double()).sum().backward()
        out[f"{case}.y"], out[f"{case}.dx"] = t.detach().numpy(), xr.grad.numpy()
        for tag, _, _, m in mods:
            for n, p in m.named_parameters():
                if p.numel() > C.PROBE_ABOVE:
                    for k, v in C.probe(p.grad).items():
                        out[f"{case}.grad.{tag}.{n}.{k}"] = v.numpy()
                else:
                    out[f"{case}.grad.{tag}.{n}"] = p.grad.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
