#!/usr/bin/env python3
"""Generate tests/golden/golden_flow_voxel.npz and flow_voxel_signatures.json by running the REFERENCE's time-aware flow functions
(src/utils/flow_utils.py:49-702) on small seeded flows.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_flow_voxel.py

``flow_utils.py`` is loaded alone (importing ``src.utils`` as a package would pull in every third-party module the reference's other
utilities need); ``cv2``, which it imports and these functions never call, stands in as an empty module.  Only arrays and names go
into the fixture.

Inputs: B = 2 flows of 6 x 7 in [-3, 3] with both signs and exact zeros, float64 and the same values in float32.
  step_<scheme>_<k>_<np|t64|t32>      one step, (dt, dx, dy) = STEPS[k], of the 4-D batch
  vox_<scheme>_<T>_<loc>_<np|t64|t32> the constructors (upwind, burgers), clamp None
  voxc_...                            the same with clamp = 1 (T = 5, middle)
  bil_<k>_<np|t64|t32>                propagate_flow_to_voxel(flow[0], DTS[k], "bilinear")
  trunc                               truncate_voxel_flow_numpy of an upwind voxel with some pixels zeroed in some bins
"""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

B, H, W = 2, 6, 7
STEPS = [(0.2, 1, 1), (-0.25, 2, 4)]
DTS = [0.4, -0.7]
BINS = (1, 2, 3, 5)
NAMES = ("construct_dense_flow_voxel_numpy", "construct_dense_flow_voxel_torch", "propagate_flow_to_voxel_numpy",
         "propagate_flow_to_voxel_torch", "upwind_flow_to_voxel_numpy", "upwind_flow_to_voxel_torch",
         "inviscid_burger_flow_to_voxel_numpy", "inviscid_burger_flow_to_voxel_torch", "truncate_voxel_flow_numpy",
         "convert_flow_per_bin_to_flow_per_sec")


def load_flow_utils():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_flow_utils", f"{REF}/src/utils/flow_utils.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def flows():
    rs = np.random.RandomState(5101)
    f = rs.uniform(-3.0, 3.0, (B, 2, H, W))
    f[rs.uniform(size=f.shape) < 0.15] = 0.0
    return f


def params_of(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def main():
    ref = load_flow_utils()
    f64 = flows()
    variants = {"np": f64, "t64": torch.from_numpy(f64), "t32": torch.from_numpy(f64.astype(np.float32))}
    out = {"flows": f64}

    def arr(a):
        return a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    steps = {"upwind": (ref.upwind_flow_to_voxel_numpy, ref.upwind_flow_to_voxel_torch),
             "burgers": (ref.inviscid_burger_flow_to_voxel_numpy, ref.inviscid_burger_flow_to_voxel_torch)}
    for scheme, fns in steps.items():
        for k, (dt, dx, dy) in enumerate(STEPS):
            for v, f in variants.items():
                out[f"step_{scheme}_{k}_{v}"] = arr(fns[v != "np"](f, dt, dx, dy))
    ctor = {"np": ref.construct_dense_flow_voxel_numpy, "t64": ref.construct_dense_flow_voxel_torch, "t32": ref.construct_dense_flow_voxel_torch}
    for scheme in steps:
        for T in BINS:
            for loc in ("first", "middle"):
                for v, f in variants.items():
                    out[f"vox_{scheme}_{T}_{loc}_{v}"] = arr(ctor[v](f, T, scheme, loc))
        for v, f in variants.items():
            out[f"voxc_{scheme}_5_middle_{v}"] = arr(ctor[v](f, 5, scheme, "middle", 1))
    for k, dt in enumerate(DTS):
        for v, f in variants.items():
            fn = ref.propagate_flow_to_voxel_numpy if v == "np" else ref.propagate_flow_to_voxel_torch
            out[f"bil_{k}_{v}"] = arr(fn(f[0], dt, "bilinear"))
    voxel = np.array(out["vox_upwind_5_middle_np"][0])
    voxel[1, :, 2, 3] = 0.0
    voxel[:, :, 4, 1] = 0.0
    voxel[3, 0, 0, 0] = 0.0
    out["trunc_in"] = voxel
    out["trunc"] = ref.truncate_voxel_flow_numpy(voxel)

    with open(os.path.join(HERE, "flow_voxel_signatures.json"), "w") as fh:
        json.dump({n: {"params": params_of(getattr(ref, n))} for n in NAMES}, fh, indent=1, sort_keys=True)
    path = os.path.join(HERE, "golden_flow_voxel.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(out)} arrays")


if __name__ == "__main__":
    main()
