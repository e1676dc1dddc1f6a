#!/usr/bin/env python3
"""Generate tests/golden/golden_photometric.npz and photometric_signatures.json by running the REFERENCE's own ``warp_image_forward``,
``warp_image_torch`` (src/utils/frame_utils.py:56-115), ``ssim`` and ``create_window`` (src/utils/stat_utils.py:215-285) on the seeded
cases of tests/_photometric_cases.py.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_photometric.py

Stored, all float64 (a float32 result is stored exactly), outputs only -- the inputs are rebuilt from seeds:
  <warp case>_np        warp_image_forward on numpy arrays (the reference computes in float64), for GOLDEN_WARP_NUMPY
  <warp case>_f64, _f32 warp_image_forward on tensors of that dtype (a uint8 image is cast first: grid_sample takes no uint8);
                        float64 alone for GOLDEN_WARP_F64_ONLY
  <shift case>_f64, _f32  warp_image_torch of the float64 image with the shift in that dtype
  <ssim case>_f64, _f32   ssim(size_average=True) followed by the B values of ssim(size_average=False)
  window_<n>            create_window(n, 1)[0, 0] for n = 5, 11, 13
and, in the JSON, the parameters (name, kind, default) of the five reference callables.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
from _photometric_cases import (GOLDEN_WARP, GOLDEN_WARP_F64_ONLY, GOLDEN_WARP_NUMPY, SHIFT_CASES, SSIM_CASES, shift_inputs, ssim_inputs, warp_inputs)  # noqa: E402

DTYPES = (("f64", torch.float64), ("f32", torch.float32))


def parameters(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def main():
    import_reference()   # (stubs cv2, openpiv, ... so that src.utils imports)
    from src.utils import SSIM, warp_image_forward, warp_image_torch
    from src.utils.stat_utils import create_window, ssim   # (src.utils exports the class only)
    out = {}
    for name in GOLDEN_WARP:
        im, flow = warp_inputs(name)
        if name in GOLDEN_WARP_NUMPY:
            out[name + "_np"] = warp_image_forward(im, flow).astype(np.float64)
        for tag, dt in DTYPES[:1] if name in GOLDEN_WARP_F64_ONLY else DTYPES:
            out[f"{name}_{tag}"] = warp_image_forward(torch.from_numpy(im).to(dt), torch.from_numpy(flow).to(dt)).double().numpy()
    for name in SHIFT_CASES:
        im, shift = shift_inputs(name)
        for tag, dt in DTYPES:
            out[f"{name}_{tag}"] = warp_image_torch(torch.from_numpy(im), torch.from_numpy(shift).to(dt)).double().numpy()
    for name, (B, C, _, _, ws) in SSIM_CASES.items():
        a, b = ssim_inputs(name)
        for tag, dt in DTYPES:
            x, y = torch.from_numpy(a).to(dt), torch.from_numpy(b).to(dt)
            out[f"{name}_{tag}"] = np.concatenate([ssim(x, y, ws, True).double().reshape(1).numpy(), ssim(x, y, ws, False).double().numpy()])
    for ws in (5, 11, 13):
        w = create_window(ws, 1)
        assert w.dtype == torch.float32 and tuple(w.shape) == (1, 1, ws, ws)
        out[f"window_{ws}"] = w[0, 0].double().numpy()
    path = os.path.join(HERE, "golden_photometric.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")
    sigs = {"warp_image_forward": parameters(warp_image_forward), "warp_image_torch": parameters(warp_image_torch),
            "ssim": parameters(ssim), "SSIM": parameters(SSIM.__init__), "SSIM.forward": parameters(SSIM.forward)}
    path = os.path.join(HERE, "photometric_signatures.json")
    with open(path, "w") as f:
        json.dump(sigs, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
