#!/usr/bin/env python3
"""Generate tests/golden/svtr.npz by running the REFERENCE MultiHeadSelfAttention, MixingBlock, Merging and Combining
(model_sgm_mms_svtr/model/svtr.py, torch only) on the CPU in float64.  Runs only where the reference is checked out; the
fixture holds data only.
Stored:
  init.{attn,block,merge,comb}.*  the four modules of svtr_cases.INIT, each after manual_seed(123): state_dict keys, shapes,
                        per-key sums
  sd.{attn,block,merge,comb}.*    their perturbed state_dicts (swin_cases.perturb), float32 as stored
  {case}.xsum, .dysum   float64 sums of the float32 inputs of svtr_cases.inputs (seeded: the tests regenerate them)
  {case}.sums.{tag}.*   float64 sum of every state_dict entry of the case's modules (svtr_cases.case_modules rebuilds them
                        from their seeds; the sums tell a rebuilt module from the one that ran here)
  {case}.y, .dx         the output and the input gradient of sum(y * dy), float64
  {case}.grad.{tag}.*   every parameter gradient; one of more than svtr_cases.PROBE_ABOVE elements as .gv / .ug / .max
                        (swin_cases.probe)
  mask.{H}x{W}.{kh}x{kw}  the fork's build_local_mask as a packed bit matrix (1 = visible), for the box arithmetic of
                        tests/svtr_refs.py
The limitation of tools/make_goldens_swin.py holds here too: a case's modules are rebuilt from torch's CPU sampling streams.
    python tools/make_goldens_svtr.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "svtr.npz")
MASKS = [(16, 24, 7, 11), (4, 12, 7, 11), (9, 37, 7, 11), (8, 40, 3, 5), (3, 70, 1, 11), (20, 3, 7, 1), (2, 3, 7, 11)]


def _load(ref):
    spec = importlib.util.spec_from_file_location("ref_svtr_model", os.path.join(ref, "model_sgm_mms_svtr", "model", "svtr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import svtr_cases as C
    if len(sys.argv) != 2:
        sys.exit("usage: make_goldens_svtr.py <checkout of the reference, the directory that holds model_sgm_mms_svtr>")
    M = _load(sys.argv[1])
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

    for H, W, kh, kw in MASKS:
        out[f"mask.{H}x{W}.{kh}x{kw}"] = np.packbits((M.build_local_mask(H, W, kh, kw) == 0).numpy())

    for case, (B, H, W, _, _) in C.CASES.items():
        x, dy = C.inputs(case)
        out[f"{case}.xsum"], out[f"{case}.dysum"] = np.array(float(x.double().sum())), np.array(float(dy.double().sum()))
        mods = C.case_modules(M, case)
        for tag, _, _, m in mods:
            for k, v in m.state_dict().items():
                out[f"{case}.sums.{tag}.{k}"] = np.array(float(v.double().sum()))
            m.double().eval()            # Combining's Dropout: the identity
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
