#!/usr/bin/env python3
"""Generate tests/golden/van.npz by running the REFERENCE VANHeightReducer and HorizontalMixer
(model_sgm_mms_attach_van/model/HTR_VT.py; the copy in model_sgm_mms_attach_van_2 is identical) on the CPU in float64, with
the timm stand-in of tools/make_goldens.py.  Runs only where the reference is checked out; the fixture holds data only.
Stored:
  init.{reducer,hmix}.*  VANHeightReducer(32, depth=2) / HorizontalMixer(32, 9), each after manual_seed(123): state_dict
                         keys, shapes, per-key sums
  sd.van_reducer.* / sd.hmix.*   the perturbed state_dicts (tests/van_cases.perturb of those seed-123 modules), float32,
                         under the names of a fork checkpoint: the modules of every case
  {case}.x, .dy, .xm, .dym       the float32 inputs of van_cases.inputs
  {case}.{red,mix}.*     y_eval, y_train, dx and grad.* (backward of sum(y_train * dy)), buf.* = every BatchNorm buffer
                         after the train forward (float64)
  {case}.red.gradscale.blocks.i.proj2.bias   max over channels of sum |d norm input|: proj2.bias feeds a train-mode
                         BatchNorm, so its gradient is a sum that cancels to rounding noise (1e-17 here); errors of
                         that gradient are measured against the magnitude of the terms of the sum
    python tools/make_goldens_van.py
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
OUT = os.path.join(ROOT, "tests", "golden", "van.npz")
REF = "/root/reference/model_sgm_mms_attach_van"


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


def _run(out, pre, m, x, dy, scales=()):
    """eval forward, train forward + backward of a float64 module -> out[pre + ...]"""
    with torch.no_grad():
        out[pre + "y_eval"] = m.eval()(x.double()).numpy()
    seen = {}

    def keep(name):
        def hook(_module, args):
            args[0].retain_grad()
            seen[name] = args[0]
        return hook
    hooks = [mod.register_forward_pre_hook(keep(n)) for n, mod in scales]
    xr = x.double().requires_grad_(True)
    y = m.train()(xr)
    (y * dy.double()).sum().backward()
    for h in hooks:
        h.remove()
    out[pre + "y_train"] = y.detach().numpy()
    out[pre + "dx"] = xr.grad.numpy()
    for n, p in m.named_parameters():
        out[pre + "grad." + n] = p.grad.numpy()
    for n, b in m.named_buffers():
        out[pre + "buf." + n] = b.numpy().copy()
    for n, t in seen.items():
        out[pre + "gradscale." + n] = np.array(float(t.grad.abs().sum((0, 2, 3)).max()))


def main():
    from make_goldens import _install_timm_stub
    import van_cases as C
    _install_timm_stub()
    M = _load("ref_van_model", "model/HTR_VT.py")
    build = {"reducer": lambda: M.VANHeightReducer(C.D, depth=C.DEPTH), "hmix": lambda: M.HorizontalMixer(C.D, k=C.K)}
    out, base = {}, {}
    for tag, ctor in build.items():
        torch.manual_seed(C.INIT_SEED)
        sd = ctor().state_dict()
        out[f"init.{tag}.keys"] = np.array(list(sd.keys()))
        out[f"init.{tag}.shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        out[f"init.{tag}.sums"] = np.array([float(v.double().sum()) for v in sd.values()])
        torch.manual_seed(C.INIT_SEED)
        base[tag] = C.perturb(ctor()).state_dict()
    for k, v in base["reducer"].items():
        out["sd.van_reducer." + k] = v.numpy().copy()
    for k, v in base["hmix"].items():
        out["sd.hmix." + k] = v.numpy().copy()

    for case in C.CASES:
        x, dy, xm, dym = C.inputs(case)
        for n, t in (("x", x), ("dy", dy), ("xm", xm), ("dym", dym)):
            out[f"{case}.{n}"] = t.numpy()
        red = ctor_load(build["reducer"], base["reducer"])
        _run(out, case + ".red.", red, x, dy, scales=[(f"blocks.{i}.proj2.bias", b.norm) for i, b in enumerate(red.blocks)])
        _run(out, case + ".mix.", ctor_load(build["hmix"], base["hmix"]), xm, dym)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


def ctor_load(ctor, sd):
    m = ctor()
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.double()


if __name__ == "__main__":
    main()
