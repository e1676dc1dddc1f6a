#!/usr/bin/env python3
"""Generate tests/golden/golden_eklt.npz by running the REFERENCE's sampled EKLT solvers, ``PatchEklt`` (src/solver/patch_eklt.py)
and ``GenerativeMaximumLikelihood`` (src/solver/generative_max_likelihood.py), on the seeded cases of tests/_eklt_cases.py.  Runs
only where the reference is checked out, with the shims of make_golden_gml.py (OpenCV restated in numpy, torchvision's resize by
F.interpolate, a no-op visualiser) and two more:

* ``cv2.warpPerspective`` is tests/_eklt_warp64.py's float64 restatement of OpenCV's classic path;
* ``optuna`` is the stub below: a study feeds a PREPARED trial list to the objective, one ``suggest_float`` per parameter, and
  keeps the first minimum (a NaN value never wins).  Every study of an ``estimate`` call gets the same list -- the table
  tests/_eklt_ref.py's ``sampler_table`` draws from numpy's global RandomState once per call -- because the reference's own stream
  (a fresh optuna sampler per patch) cannot be pinned without optuna.  A study none of whose values is a number (the zero-histogram
  box of the ``thres`` case, where the reference divides by zero) reports all-zero parameters.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eklt.py

Stored per case: ``<case>_cost`` [P, K] (the reference's ``_objective_optuna`` on its own ``_make_measured_increment`` for every
patch and every row of ``hypotheses(case)``; NaN rows for the zero-histogram box), ``<case>_margin`` (the smallest relative lead of
the largest column sum of |Q - P|), ``<case>_selected`` (np.packbits of the patches ``estimate`` optimised), ``<case>_best`` (the
winning trial per patch, -1 where none), ``<case>_best_value``, ``<case>_flow`` (the rows ``stored_rows(case)`` of the returned
flow) and ``<case>_flow_absmax``.  The generator asserts that every 32 p of a table is at least 1e-6 from a half-integer and that
every margin exceeds 1e-9, and prints the worst of both.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from make_golden import import_reference, install_torchvision_shim  # noqa: E402
from make_golden_gml import MARGIN_MIN, _NoViz, install_cv2_shim  # noqa: E402
import _eklt_ref as E  # noqa: E402
from _eklt_cases import CASES, ZERO_NORM_BOX, case_inputs, hypotheses, solver_config, stored_rows  # noqa: E402
from _eklt_warp64 import half_integer_margin, warp_perspective_f64  # noqa: E402

HALF_MARGIN_MIN = 1e-6


class _Trial(object):
    def __init__(self, number, params):
        self.number, self.params, self.asked = number, params, []

    def suggest_float(self, key, low, high):
        v = float(self.params[key])
        assert low <= v <= high, (key, v, low, high)
        self.asked.append(key)
        return v


class _Study(object):
    """The stub study: ``trials`` is the prepared list of {parameter: value}."""
    trials = []      # set by the generator before every estimate call
    log = []         # (best trial or -1) of every study opened since the generator cleared it

    def __init__(self):
        self.best_params, self.best_value, self.best_number = None, float("nan"), -1

    def optimize(self, objective, n_trials):
        assert n_trials == len(self.trials), (n_trials, len(self.trials))
        for i, params in enumerate(self.trials):
            trial = _Trial(i, params)
            with np.errstate(all="ignore"):
                v = float(objective(trial))
            assert trial.asked == list(params), (trial.asked, list(params))   # one suggest_float per parameter, in order
            if v == v and (self.best_number < 0 or v < self.best_value):
                self.best_params, self.best_value, self.best_number = dict(params), v, i
        if self.best_number < 0:
            self.best_params = {k: 0.0 for k in self.trials[0]}
        _Study.log.append(self.best_number)


def install_optuna_stub():
    op = types.ModuleType("optuna")
    op.Trial = _Trial
    op.samplers = types.SimpleNamespace(TPESampler=lambda **k: "TPE", RandomSampler=lambda **k: "random",
                                        GridSampler=lambda space, **k: ("grid", space))
    op.create_study = lambda direction, sampler, storage: _Study()
    return op


def trials_of(cfg, table):
    keys = list(cfg["optimizer"]["parameters"])
    return [dict(zip(keys, (float(v) for v in row))) for row in table]


def cost_tables(solver, name, events):
    """_objective_optuna on _make_measured_increment for every patch (or the ROI) and every row of the case's table."""
    cfg = solver.slv_config
    trials = trials_of(cfg, hypotheses(name))
    if CASES[name]["kind"] == "patch":
        solver.calculate_iwe_cache(events)
        rois = [solver.patches[i] for i in range(solver.n_patch)]
    else:
        rois = [{k: cfg["filter"]["parameters"][k] for k in ("xmin", "xmax", "ymin", "ymax")}]
    cost, margin = np.full((len(rois), len(trials)), np.nan), 1.0
    last = {}
    predict = solver._make_prediction_numpy

    def _predict(parameters, roi, weights):
        last["P"] = predict(parameters, roi, weights)
        return last["P"]

    solver._make_prediction_numpy = _predict
    zero = ZERO_NORM_BOX.get(name)
    for i, roi in enumerate(rois):
        if zero is not None and (roi["xmin"], roi["xmax"], roi["ymin"], roi["ymax"]) == zero:
            continue
        with np.errstate(all="ignore"):
            Q, weights = solver._make_measured_increment(events, roi)
        if not np.isfinite(Q).all():
            continue
        Q = Q.copy()
        for k, params in enumerate(trials):
            cost[i, k] = solver._objective_optuna(_Trial(k, params), Q, roi, weights)
            margin = min(margin, E.column_margin(last["P"], Q))
    solver._make_prediction_numpy = predict
    return cost, margin


def run_case(name, classes):
    c = CASES[name]
    H, W = c["shape"]
    frame, events = case_inputs(name)
    cfg = solver_config(name)
    cls = classes[c["kind"]]
    solver = cls((H, W), (H, W), {}, cfg, _NoViz())
    solver._set_frame(frame)
    cost, margin = cost_tables(solver, name, events)
    # estimate: a fresh solver (the cost tables divided the patch solver's cached histogram in place)
    solver = cls((H, W), (H, W), {}, solver_config(name), _NoViz())
    np.random.seed(c["init_seed"])
    table = E.sampler_table(cfg["optimizer"])
    _Study.trials, _Study.log = trials_of(cfg, table), []
    estimated = []
    patch_estimate = solver._estimate_patch

    def _estimate_patch(ev, roi):
        if c["kind"] == "patch":
            estimated.append([k for k in range(solver.n_patch) if solver.patches[k] is roi][0])
        return patch_estimate(ev, roi)

    solver._estimate_patch = _estimate_patch
    with np.errstate(all="ignore"):
        flow = np.asarray(solver.estimate(events, frame=frame, background=frame))
    n = solver.n_patch if c["kind"] == "patch" else 1
    if c["kind"] != "patch":
        estimated = [0]
    sel, best = np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int64)
    sel[estimated] = True
    best[estimated] = _Study.log
    p_all = np.concatenate([E.unfold(cfg["generative_ml"], list(c["params"]), t)[:, 2:].reshape(-1) for t in (hypotheses(name), table)])
    return cost, margin, sel, best, flow, float(half_integer_margin(p_all).min())


def main():
    cv2 = install_cv2_shim()
    cv2.warpPerspective = lambda src, M, dsize, **kw: warp_perspective_f64(src, M, dsize)
    import_reference()
    install_torchvision_shim()
    sys.modules["cv2"] = cv2
    import src.solver.patch_eklt as rpe
    import src.solver.generative_max_likelihood as rgml

    rpe.cv2 = rgml.cv2 = cv2
    rpe.transforms = sys.modules["torchvision.transforms"]
    rgml.visualizer = types.SimpleNamespace(Visualizer=_NoViz)
    rgml.optuna = rpe.optuna = install_optuna_stub()
    classes = {"patch": rpe.PatchEklt, "global": rgml.GenerativeMaximumLikelihood}
    out = {"shimmed": np.array(1)}
    for name in CASES:
        cost, margin, sel, best, flow, half = run_case(name, classes)
        assert margin > MARGIN_MIN, (name, margin)
        assert half >= HALF_MARGIN_MIN, (name, half)
        out[name + "_cost"] = cost
        out[name + "_margin"] = np.array(margin)
        out[name + "_selected"] = np.packbits(sel)
        out[name + "_best"] = best.astype(np.int32)
        out[name + "_flow"] = flow[:, stored_rows(name)]
        out[name + "_flow_absmax"] = np.abs(flow).max()
        print(f"{name:14s} boxes {len(sel):3d}  selected {int(sel.sum()):3d}  K {cost.shape[1]:3d}  cost {np.nanmin(cost):.4f} .. {np.nanmax(cost):.4f}"
              f"  min column margin {margin:.2e}  min |32 p - half| {half:.2e}  max|flow| {np.abs(flow).max():.4g}", flush=True)
    path = os.path.join(HERE, "golden_eklt.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    warnings.filterwarnings("ignore")
    main()
