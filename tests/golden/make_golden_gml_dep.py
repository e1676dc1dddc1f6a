#!/usr/bin/env python3
"""Generate tests/golden/golden_gml_dep.npz by running the REFERENCE's single-scale generative solver,
``PatchEkltDependent.estimate`` (src/solver/patch_eklt_dependent.py on patch_eklt.py, generative_max_likelihood.py), on the
seeded cases of tests/_gml_dep_cases.py.  Runs only where the reference is checked out, with the shims of make_golden_gml.py
(OpenCV restated in numpy, torchvision's resize by F.interpolate, a no-op visualiser):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gml_dep.py

Stored per case: ``<case>_loss`` and ``<case>_<term>`` (cost_func.get_history(), one value per Adam iteration),
``<case>_selected`` (estimate_indices as a bit mask over the row-major patch grid, np.packbits), ``<case>_x`` (the grid rows
``stored_param_rows(case)`` of the final parameters as the [n_dim, gh, gw] grid), ``<case>_flow`` (the rows ``stored_rows(case)`` of the returned [2, H, W]
flow), ``<case>_flow_absmax`` and ``<case>_margin``: per iteration, (largest - second largest) / largest column sum of |Q - P|.
The generator asserts margin > 1e-9 (no near-ties between diff_norm's columns).
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from make_golden import import_reference, install_torchvision_shim  # noqa: E402
from make_golden_gml import MARGIN_MIN, _NoViz, install_cv2_shim  # noqa: E402
import _gml_dep_ref as D  # noqa: E402
from _gml_dep_cases import CASES, case_inputs, solver_config, stored_param_rows, stored_rows  # noqa: E402


def run_case(name, cls):
    c = CASES[name]
    H, W = c["shape"]
    frame, events = case_inputs(name)
    viz = _NoViz()
    solver = cls((H, W), (H, W), {}, solver_config(name), viz)
    margins, last = [], {}
    calc = solver._calculate_cost

    def _calculate_cost(measured, predicted, **kw):
        with torch.no_grad():
            cs = torch.abs(measured - predicted).sum(0)
            top = torch.topk(cs, 2).values
            margins.append(float((top[0] - top[1]) / top[0]))
        return calc(measured, predicted, **kw)

    extrapolate = solver._extrapolate_dense_flow_from_estimates

    def _extrapolate(parameters, *args):
        last["x"] = parameters.detach().clone()
        return extrapolate(parameters, *args)

    solver._calculate_cost = _calculate_cost
    solver._extrapolate_dense_flow_from_estimates = _extrapolate
    np.random.seed(c["init_seed"])
    flow = solver.estimate(events, frame=frame, background=frame)
    idx = np.asarray(solver.estimate_indices, dtype=np.int64)
    nd = solver.n_parameter_dim
    gh, gw = solver.patch_image_size
    grid = np.zeros((nd, gh * gw))
    grid[:, idx] = last["x"].cpu().numpy().reshape(-1, nd).T
    return viz.history, idx, grid.reshape(nd, gh, gw), np.asarray(flow), np.array(margins)


def main():
    cv2 = install_cv2_shim()
    import_reference()
    install_torchvision_shim()
    sys.modules["cv2"] = cv2
    import src.solver.patch_eklt as rpe
    import src.solver.patch_eklt_dependent as rpd
    import src.solver.generative_max_likelihood as rgml

    rpe.cv2 = rpd.cv2 = rgml.cv2 = cv2
    rpe.transforms = sys.modules["torchvision.transforms"]
    rgml.visualizer = types.SimpleNamespace(Visualizer=_NoViz)
    only = sys.argv[1:]
    out = {"shimmed": np.array(1)}
    for name in CASES:
        if only and name not in only:
            continue
        hist, idx, grid, flow, margins = run_case(name, rpd.PatchEkltDependent)
        assert margins.min() > MARGIN_MIN, (name, margins.min())
        out[name + "_loss"] = np.array(hist["loss"])
        for k in CASES[name]["cost"]:
            out[f"{name}_{k}"] = np.array(hist[k])
        mask = np.zeros(grid.shape[1] * grid.shape[2], dtype=bool)
        mask[idx] = True
        out[name + "_selected"] = np.packbits(mask)
        out[name + "_x"] = grid[:, stored_param_rows(name)]
        out[name + "_flow"] = flow[:, stored_rows(name)]
        out[name + "_flow_absmax"] = np.abs(flow).max()
        out[name + "_margin"] = margins
        print(f"{name:16s} iters {len(hist['loss'])}  selected {len(idx)} of {grid.shape[1] * grid.shape[2]}  loss {hist['loss'][0]:.6f}"
              f" -> {hist['loss'][-1]:.6f}  min margin {margins.min():.2e}  max|flow| {np.abs(flow).max():.4g}", flush=True)
    path = os.path.join(HERE, "golden_gml_dep.npz" if not only else "golden_gml_dep_partial.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    warnings.filterwarnings("ignore")
    main()
