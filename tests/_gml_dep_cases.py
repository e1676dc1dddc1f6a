"""Seeded cases of the single-scale generative solver, patch_eklt_dependent (tests/golden/golden_gml_dep.npz; tests/test_gml_dep.py,
tests/test_gpu_gml_dep.py).

A case is a window of synthetic events over a textured frame (tests/_gml_cases.py), a ROI, the reference's ``generative_ml`` and
``patch_eklt`` options and ``n_iter``.  ``solver_config(name)`` is the ``solver`` section the reference's ``PatchEkltDependent``
and this package's ``GenerativePatchDependent`` are constructed with.  The initial potentials are drawn from numpy's global
RandomState, seeded with ``CASES[name]["init_seed"]`` just before ``estimate``.
"""
import copy

import numpy as np

from _gml_cases import YAML_COST, YAML_GML, frame_image, synth_events

YAML_PATCH = {"patch_size": 4, "sliding_window": 2, "do_event_thresholding": False, "event_thres": 8}   # configs/hot_plate1.yaml


def _case(shape, roi, n_iter, n_events, seed, gml=None, cost=None, patch=None, clustered=False):
    g = dict(YAML_GML)
    g.update(gml or {})
    pe = dict(YAML_PATCH)
    pe.update(patch or {})
    return {"shape": shape, "roi": roi, "n_iter": n_iter, "n_events": n_events, "seed": seed, "init_seed": 2000 + seed, "gml": g,
            "cost": dict(cost or YAML_COST), "patch": pe, "clustered": clustered}


NOWARP_COST = {"diff_norm": 1.0, "image_gradient": 0.5}

CASES = {
    "yaml_128": _case((128, 160), None, 120, 20000, 1),
    "yaml_128_roi": _case((128, 160), (16, 112, 32, 120), 120, 20000, 2),
    "nowarp_128": _case((128, 160), (8, 120, 0, 160), 120, 20000, 3, {"optimize_warp": False}, NOWARP_COST),
    "vel_128": _case((128, 160), (16, 112, 32, 120), 120, 20000, 4, {"poisson_model": False}),
    "vel_nowarp_128": _case((128, 160), None, 120, 20000, 5, {"poisson_model": False, "optimize_warp": False}, NOWARP_COST),
    "thres_128": _case((128, 160), (16, 112, 32, 120), 120, 20000, 6, None, None, {"do_event_thresholding": True}, True),
    "nopol_128": _case((128, 160), (16, 112, 32, 120), 120, 20000, 7, {"no_polarity": True}),
    "evhist_128": _case((128, 160), (16, 112, 32, 120), 120, 20000, 8, {"weight_loss_by_event_hist": True}),
    "odd_128": _case((128, 160), (10, 117, 21, 150), 120, 20000, 9, None, None, {"patch_size": 5, "sliding_window": 3}),
    "yaml_260": _case((260, 346), (0, 260, 86, 260), 60, 60000, 10),
    "yaml_720": _case((720, 1280), (0, 720, 320, 960), 6, 50000, 11),
}


def clustered_events(n, H, W, seed):
    """Events in six Gaussian blobs (integer pixels), so that event thresholding drops most patches."""
    rs = np.random.RandomState(seed)
    centres = np.stack([rs.uniform(0.2 * H, 0.8 * H, 6), rs.uniform(0.2 * W, 0.8 * W, 6)], axis=1)
    which = rs.randint(0, 6, n)
    xy = centres[which] + rs.normal(0.0, 5.0, (n, 2))
    x = np.clip(np.round(xy[:, 0]), 0, H - 1)
    y = np.clip(np.round(xy[:, 1]), 0, W - 1)
    t = np.sort(rs.uniform(0.0, 0.05, n))
    p = rs.randint(0, 2, n)
    return np.stack([x, y, t, p], axis=1).astype(np.float64)


def case_inputs(name):
    """-> (frame [H, W] float64, events [n, 4] float64 (x = row, y = column, t, p))."""
    c = CASES[name]
    H, W = c["shape"]
    ev = (clustered_events if c["clustered"] else synth_events)(c["n_events"], H, W, 300 + c["seed"])
    return frame_image(H, W, 100 + c["seed"]), ev


def roi_of(name):
    c = CASES[name]
    H, W = c["shape"]
    return c["roi"] if c["roi"] is not None else (0, H, 0, W)


def geometry(name):
    """-> (patch, slide, thresholding, event_thres)."""
    pe = CASES[name]["patch"]
    return pe["patch_size"], pe["sliding_window"], pe["do_event_thresholding"], pe["event_thres"]


def solver_config(name, **gml_overrides):
    """The reference YAML's ``solver`` section for the case (method patch_eklt_dependent)."""
    c = CASES[name]
    xmin, xmax, ymin, ymax = roi_of(name)
    g = copy.deepcopy(c["gml"])
    g.update(gml_overrides)
    return {
        "method": "patch_eklt_dependent",
        "filter": {"filters": [], "parameters": {"xmin": xmin, "xmax": xmax, "ymin": ymin, "ymax": ymax}},
        "warp_direction": "first", "motion_model": "2d-translation", "parameters": ["trans_x", "trans_y"], "cost": "hybrid",
        "outer_padding": 0, "cost_with_weight": dict(c["cost"]),
        "iwe": {"method": "bilinear_vote", "blur_sigma": 3},
        "optimizer": {"method": "Adam", "n_iter": c["n_iter"],
                      "parameters": {"angle": {"min": 0, "max": 6.2832}, "p_x": {"min": -0.4, "max": 0.4},
                                     "p_y": {"min": -0.4, "max": 0.4}}},
        "generative_ml": g,
        "patch_eklt": dict(c["patch"]),
    }


def stored_rows(name):
    """The rows of the output flow the fixture keeps: every 32nd at 128 x 160, every 64th at 260 x 346, every 360th at 720 x 1280
    (float64 flows do not compress, and the fixture stays small)."""
    H = CASES[name]["shape"][0]
    return np.arange(0, H, 360 if H >= 720 else (64 if H >= 260 else 32))


def stored_param_rows(name):
    """The grid rows of the final parameters the fixture keeps: every 16th at 128 x 160, every 32nd at 260 x 346, every 120th at
    720 x 1280."""
    H = CASES[name]["shape"][0]
    p, s = CASES[name]["patch"]["patch_size"], CASES[name]["patch"]["sliding_window"]
    gh = len(np.arange(0, H - p + s, s))
    return np.arange(0, gh, 120 if H >= 720 else (32 if H >= 260 else 16))
