#!/usr/bin/env python3
"""Generate tests/golden/golden_voxel.npz and voxel_signatures.json by running the REFERENCE's ``create_event_voxel`` and
``generate_discretized_event_volume`` (src/utils/event_utils.py:291-440) on small seeded inputs.  Runs only where the reference is
checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_voxel.py

``event_utils.py`` is loaded alone, under stand-in parent packages: importing ``src.utils`` as a package would pull in every
third-party module the reference's other utilities need.  Its one relative import, ``..types``, is given the four names it asks
for.  Only arrays and names go into the fixture.

Cases (a 12 x 16 sensor, C = 5, about 2000 events with strictly increasing times):
  int    integer pixels, both polarities
  frac   fractional pixels, with coordinates in (-1, 0) and beyond W - 1 / H - 1
  pos    positive polarity only, un-normalised and with normalize=True
  vol    the discretised volume, T = 6, both polarities, float64 and float32 events
"""
import importlib.util
import inspect
import json
import os
import sys
import types
from typing import Union

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

H, W, C, N, T = 12, 16, 5, 2000, 6


def load_event_utils():
    for name in ("refsrc", "refsrc.utils"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    ty = types.ModuleType("refsrc.types")
    ty.NUMPY_TORCH = Union[np.ndarray, torch.Tensor]
    ty.FLOAT_TORCH = Union[float, torch.Tensor]
    ty.is_torch = lambda a: isinstance(a, torch.Tensor)
    ty.is_numpy = lambda a: isinstance(a, np.ndarray)
    sys.modules["refsrc.types"] = ty
    spec = importlib.util.spec_from_file_location("refsrc.utils.event_utils", f"{REF}/src/utils/event_utils.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def times(rs, n):
    return np.cumsum(rs.uniform(1e-6, 1e-5, n)) + 0.25        # strictly increasing


def params_of(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def main():
    ref = load_event_utils()
    out = {"shape": np.array([C, H, W]), "vol_size": np.array([T, H, W])}

    def voxel(x, y, pol, t, normalize=False):
        g = ref.create_event_voxel(*(torch.from_numpy(a) for a in (x, y, pol, t)), (C, H, W), normalize)
        assert g.dtype == torch.float64 and tuple(g.shape) == (C, H, W)
        return g.numpy()

    rs = np.random.RandomState(4101)
    x, y = rs.randint(0, W, N).astype(np.float64), rs.randint(0, H, N).astype(np.float64)
    pol, t = rs.randint(0, 2, N) * 2.0 - 1.0, times(rs, N)
    out.update(int_x=x, int_y=y, int_pol=pol, int_t=t, int_grid=voxel(x, y, pol, t))

    rs = np.random.RandomState(4102)
    x, y = rs.uniform(-1.0, W + 0.5, N), rs.uniform(-1.0, H + 0.5, N)
    x[:40], y[40:80] = rs.uniform(-1.0, 0.0, 40), rs.uniform(-1.0, 0.0, 40)
    x[80:120], y[120:160] = rs.uniform(W - 1, W, 40), rs.uniform(H - 1, H, 40)
    pol, t = rs.randint(0, 2, N) * 2.0 - 1.0, times(rs, N)
    out.update(frac_x=x, frac_y=y, frac_pol=pol, frac_t=t, frac_grid=voxel(x, y, pol, t))

    rs = np.random.RandomState(4103)
    x, y = rs.uniform(0.0, W - 1, N), rs.uniform(0.0, H - 1, N)
    pol, t = np.ones(N), times(rs, N)
    out.update(pos_x=x, pos_y=y, pos_pol=pol, pos_t=t, pos_grid=voxel(x, y, pol, t), pos_grid_normalized=voxel(x, y, pol, t, True))

    rs = np.random.RandomState(4104)
    ev = np.stack([rs.randint(0, H, N), rs.randint(0, W, N), times(rs, N), rs.randint(0, 2, N) * 2.0 - 1.0], axis=1).astype(np.float64)
    ev[5:9, :2] += 0.75                                        # .long() truncates
    out["vol_events"] = ev
    out["vol_volume"] = ref.generate_discretized_event_volume(torch.from_numpy(ev), (T, H, W)).numpy()
    ev32 = ev.astype(np.float32)
    ev32[:, 2] = (ev[:, 2] - 0.25).astype(np.float32)          # (float32 keeps the microsecond steps near 0, not near 0.25)
    out["vol32_events"] = ev32
    v32 = ref.generate_discretized_event_volume(torch.from_numpy(ev32), (T, H, W))
    assert v32.dtype == torch.float32
    out["vol32_volume"] = v32.numpy()

    with open(os.path.join(HERE, "voxel_signatures.json"), "w") as f:
        json.dump({n: {"params": params_of(getattr(ref, n))} for n in ("create_event_voxel", "generate_discretized_event_volume")},
                  f, indent=1, sort_keys=True)
    path = os.path.join(HERE, "golden_voxel.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(out)} arrays")


if __name__ == "__main__":
    main()
