#!/usr/bin/env python3
"""Generate tests/golden/golden_gml.npz by running the REFERENCE's generative solver, ``PatchEkltPyramid2.estimate``
(src/solver/patch_eklt_pyramid2.py on patch_eklt_dependent.py, patch_eklt.py, generative_max_likelihood.py), on the seeded cases
of tests/_gml_cases.py.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gml.py

OpenCV and torchvision are absent here: cv2.Sobel / GaussianBlur / resize are restated in numpy (tests/_gml_ref.py: float64,
BORDER_REFLECT_101, kernel size round(8 sigma + 1) | 1, INTER_LINEAR) and torchvision's resize by F.interpolate
(make_golden.install_torchvision_shim); the fixture carries ``shimmed = 1``.  The visualiser is a no-op object.

Stored per case: ``<case>_loss`` and ``<case>_<term>`` (cost_func.get_history(), one value per Adam iteration), ``<case>_x<s>``
(the parameters after scale s = 1..4; the grid rows ``stored_param_rows(case, s)`` where that is not None), ``<case>_flow``
(the rows ``stored_rows(case)`` of the returned [2, H, W] flow), ``<case>_flow_absmax`` and ``<case>_margin``: per iteration, (largest - second largest) / largest column sum
of |Q M - P|.  The generator asserts that margin > 1e-9, so that a float64 implementation must follow the same diff_norm
subgradient (no near-ties between columns).
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
import _gml_ref as R  # noqa: E402
from _gml_cases import CASES, case_inputs, solver_config, stored_param_rows, stored_rows  # noqa: E402

MARGIN_MIN = 1e-9


def install_cv2_shim():
    import torch.nn.functional as F

    def Sobel(src, ddepth, dx, dy, ksize=3):
        assert ksize == 3 and (dx, dy) in ((0, 1), (1, 0))
        gx, gy = R.cv_sobel(src)
        return gx if dy == 1 else gy

    def GaussianBlur(src, ksize=None, sigmaX=0.0, **kw):
        assert ksize is None and sigmaX > 0
        return R.cv_gaussian_blur(src, sigmaX)

    def resize(src, dsize, dst=None, fx=None, fy=None, interpolation=None):
        h, w = src.shape
        size = [int(round(h * fy)), int(round(w * fx))]
        t = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float64))[None, None]
        return F.interpolate(t, size=size, mode="bilinear", align_corners=False)[0, 0].numpy()

    cv2 = types.ModuleType("cv2")
    cv2.Sobel, cv2.GaussianBlur, cv2.resize = Sobel, GaussianBlur, resize
    cv2.CV_64F, cv2.INTER_LINEAR, cv2.INTER_NEAREST = 6, 1, 0
    sys.modules["cv2"] = cv2
    return cv2


class _NoViz(object):
    save_dir = "."

    def __init__(self, *a, **k):
        self.history = None

    def visualize_scipy_history(self, history):
        self.history = {k: list(v) for k, v in history.items()}

    def __getattr__(self, item):
        return lambda *a, **k: None


def run_case(name, P2, rgml):
    c = CASES[name]
    H, W = c["shape"]
    frame, events = case_inputs(name)
    viz = _NoViz()
    solver = P2((H, W), (H, W), {}, solver_config(name), viz)
    params, margins = {}, []
    run_scale = solver.run_estimation_per_scale

    def run_estimation_per_scale(ev, per_scale):
        x = run_scale(ev, per_scale)
        params[solver.current_scale] = x.reshape((-1,) + solver.patch_image_size).copy()
        return x

    calc = solver._calculate_cost

    def _calculate_cost(measured, predicted, **kw):
        with torch.no_grad():
            cs = torch.abs(measured - predicted).sum(0)
            top = torch.topk(cs, 2).values
            margins.append(float((top[0] - top[1]) / top[0]))
        return calc(measured, predicted, **kw)

    solver.run_estimation_per_scale = run_estimation_per_scale
    solver._calculate_cost = _calculate_cost
    np.random.seed(c["init_seed"])
    flow = solver.estimate(events, frame=frame, background=frame)
    return viz.history, params, np.asarray(flow), np.array(margins)


def main():
    cv2 = install_cv2_shim()
    import_reference()
    install_torchvision_shim()
    sys.modules["cv2"] = cv2
    import src.solver.patch_eklt as rpe
    import src.solver.patch_eklt_pyramid2 as rp2
    import src.solver.generative_max_likelihood as rgml

    rpe.cv2 = rp2.cv2 = rgml.cv2 = cv2
    rpe.transforms = sys.modules["torchvision.transforms"]
    rp2.resize = sys.modules["torchvision.transforms.functional"].resize
    rgml.visualizer = types.SimpleNamespace(Visualizer=_NoViz)
    out = {"shimmed": np.array(1)}
    for name in CASES:
        hist, params, flow, margins = run_case(name, rp2.PatchEkltPyramid2, rgml)
        assert margins.min() > MARGIN_MIN, (name, margins.min())
        out[name + "_loss"] = np.array(hist["loss"])
        for k in CASES[name]["cost"]:
            out[f"{name}_{k}"] = np.array(hist[k])
        for s, x in params.items():
            pr = stored_param_rows(name, s)
            out[f"{name}_x{s}"] = x if pr is None else x[:, pr]
        rows = stored_rows(name)
        out[name + "_flow"] = flow[:, rows]
        out[name + "_flow_absmax"] = np.abs(flow).max()
        out[name + "_margin"] = margins
        print(f"{name:16s} iters {len(hist['loss'])}  loss {hist['loss'][0]:.6f} -> {hist['loss'][-1]:.6f}  "
              f"min margin {margins.min():.2e}  max|flow| {np.abs(flow).max():.4g}", flush=True)
    path = os.path.join(HERE, "golden_gml.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    warnings.filterwarnings("ignore")
    main()
