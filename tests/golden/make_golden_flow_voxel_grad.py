#!/usr/bin/env python3
"""Generate tests/golden/golden_flow_voxel_grad.npz: gradients of the REFERENCE's time-aware flow (src/utils/flow_utils.py:162-224,
345-444, 502-556, 630-702) with respect to the flow at t0, taken by CPU autograd through the reference's own torch functions.  Runs
only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_flow_voxel_grad.py

``flow_utils.py`` is loaded as in make_golden_flow_voxel.py.  Only arrays and numbers go into the fixture.

The reference's constructor cannot run 'same' and 'bilinear' (it hands a 4-D batch to ``propagate_flow_to_voxel_torch``, which unpacks
three dimensions); for those the voxel is assembled here from the reference's ``propagate_flow_to_voxel_torch`` per flow and bin with
the constructor's own time offsets and clamp, which is what the product documents as its replacement.

Flows, B = 2 of 9 x 11:
  rand   in [-3, 3], both signs, 15 % exact zeros (ties of maximum / minimum)
  dense  in [-3, 3] without zeros
  pos    strictly positive and smooth: long Burgers chains keep their signs
  one    zero except for one pixel (the tie rule: the reference gives the half-and-half value)
Arrays:
  flow_<key>                       the flows, float64 (float32 cases use the same values rounded)
  up_<case>                        the upstream gradient of the voxel / the step's output: multiples of 1/16 in [-1, 1], exact in
                                   both dtypes (and small in the compressed file)
  grad_<case>_<t64|t32>            d sum(up * voxel) / d flow in that dtype
  cases                            the case names;  stable: which of them are branch-stable
  r32                              the largest max|grad_t32 - grad_t64| / max|grad_t64| over the branch-stable cases
A case is branch-stable when every bin of its float32 and float64 forward voxels has the same sign pattern; r32 is then rounding
alone.  At least one case per scheme has to be (asserted).
Case names: vox_<scheme>_<T>_<loc>_<c|n>_<key> (c: clamp 1.5), step_<scheme>_<k>_<key> with STEPS[k], prop_<method>_<k>_<key> with DTS[k]
of flow 0.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

B, H, W = 2, 9, 11
CLAMP = 1.5
STEPS = [(0.2, 1, 1), (-0.25, 2, 4), (1.0, 1, 1)]
DTS = [0.4, -0.7]
SCHEMES = ("upwind", "burgers", "same", "bilinear")
# (scheme, T, loc, clamp, flow key)
VOXELS = ([(s, T, "middle", None, k) for s in ("upwind", "burgers") for T in (5, 9, 17) for k in ("dense", "pos")]
          + [(s, T, loc, c, "rand") for s in SCHEMES for T, loc in ((5, "middle"), (4, "first"), (17, "middle")) for c in (None, CLAMP)]
          + [(s, 5, "middle", None, k) for s in ("same", "bilinear") for k in ("dense", "pos")]
          + [(s, 3, "middle", None, "one") for s in SCHEMES]
          + [("burgers", 1, "middle", None, "rand"), ("burgers", 2, "middle", CLAMP, "rand"), ("burgers", 2, "first", None, "rand"),
             ("upwind", 1, "first", CLAMP, "rand")])


def load_flow_utils():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_flow_utils", f"{REF}/src/utils/flow_utils.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def flows():
    rs = np.random.RandomState(7301)
    dense = rs.uniform(-3.0, 3.0, (B, 2, H, W))
    dense[np.abs(dense) < 0.05] = 0.05
    rand = rs.uniform(-3.0, 3.0, (B, 2, H, W))
    rand[rs.uniform(size=rand.shape) < 0.15] = 0.0
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pos = np.stack([np.stack([1.5 + 0.5 * np.sin(0.4 * ii + 0.3 * jj + b), 1.2 + 0.4 * np.cos(0.25 * ii - 0.35 * jj + 2 * b)]) for b in range(B)])
    one = np.zeros((B, 2, H, W))
    one[0, 0, 4, 5] = 1.0
    one[1, 1, 3, 6] = -2.0
    return {"rand": rand, "dense": dense, "pos": pos, "one": one}


def voxel_of(ref, f, scheme, T, loc, clamp):
    if scheme in ("upwind", "burgers"):
        return ref.construct_dense_flow_voxel_torch(f, T, scheme, loc, clamp)
    offsets = np.arange(0, T) / T if loc == "first" else (np.arange(0, T) - T // 2) / T   # the constructor's time_bin_array
    voxel = torch.stack([torch.stack([ref.propagate_flow_to_voxel_torch(f[b], offsets[i], scheme) for i in range(T)]) for b in range(B)])
    return voxel if clamp is None else torch.clamp(voxel, -clamp, clamp)


def main():
    warnings.simplefilter("ignore")
    ref = load_flow_utils()
    F = flows()
    rs = np.random.RandomState(7302)
    out = {f"flow_{k}": v for k, v in F.items()}
    names, stable = [], []

    def run(name, fn, flow, scheme):
        """fn(tensor requiring grad) -> output; both dtypes; -> is the case branch-stable"""
        res = {}
        up = None
        for tag, dt in (("t64", torch.float64), ("t32", torch.float32)):
            f = torch.from_numpy(flow).to(dt).requires_grad_()
            y = fn(f)
            if up is None:
                up = rs.randint(-16, 17, tuple(y.shape)) / 16.0
                out[f"up_{name}"] = up
            y.backward(torch.from_numpy(up).to(dt))
            assert torch.isfinite(f.grad).all(), name
            res[tag] = (y.detach().numpy(), f.grad.numpy())
            out[f"grad_{name}_{tag}"] = res[tag][1]
        names.append(name)
        stable.append(bool(np.array_equal(np.sign(res["t64"][0]), np.sign(res["t32"][0]))))
        return res

    results = {}
    for scheme, T, loc, clamp, key in VOXELS:
        name = f"vox_{scheme}_{T}_{loc}_{'n' if clamp is None else 'c'}_{key}"
        results[name] = (scheme, run(name, lambda f: voxel_of(ref, f, scheme, T, loc, clamp), F[key], scheme))
    step_fn = {"upwind": ref.upwind_flow_to_voxel_torch, "burgers": ref.inviscid_burger_flow_to_voxel_torch}
    for scheme, fn in step_fn.items():
        for k, (dt, dx, dy) in enumerate(STEPS):
            for key in ("rand", "one"):
                name = f"step_{scheme}_{k}_{key}"
                results[name] = (scheme, run(name, lambda f: fn(f, dt, dx, dy), F[key], scheme))
    for method in ("same", "bilinear"):
        for k, dt in enumerate(DTS):
            name = f"prop_{method}_{k}_rand"
            results[name] = (method, run(name, lambda f: ref.propagate_flow_to_voxel_torch(f, dt, method), F["rand"][0], method))

    r32, per_scheme = 0.0, {s: 0 for s in SCHEMES}
    for name, ok in zip(names, stable):
        if not ok:
            continue
        scheme, res = results[name]
        g64, g32 = res["t64"][1], res["t32"][1].astype(np.float64)
        rel = float(np.abs(g32 - g64).max() / np.abs(g64).max())
        print(f"{name:40s} stable  rel {rel:.3e}")
        r32 = max(r32, rel)
        per_scheme[scheme] += 1
    for name, ok in zip(names, stable):
        if not ok:
            print(f"{name:40s} NOT branch-stable")
    assert all(n > 0 for n in per_scheme.values()), per_scheme
    out["cases"] = np.array(names)
    out["stable"] = np.array(stable)
    out["r32"] = np.float64(r32)
    path = os.path.join(HERE, "golden_flow_voxel_grad.npz")
    np.savez_compressed(path, **out)
    print(f"r32 = {r32:.4e}; wrote {path} ({os.path.getsize(path)} bytes): {len(out)} arrays")


if __name__ == "__main__":
    main()
