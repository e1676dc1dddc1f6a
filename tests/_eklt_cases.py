"""Seeded cases of the sampled EKLT solvers, patch_eklt and generative_max_likelihood (tests/golden/golden_eklt.npz;
tests/test_eklt.py, tests/test_gpu_eklt.py).

A case is a window of synthetic events over a textured frame (tests/_gml_cases.py), the reference's ``generative_ml`` and
``patch_eklt`` options, the ``optimizer`` section (method optuna: sampler, n_iter, the parameters with their ranges, in order) and
an explicit hypothesis table in the configuration's parameterisation (``hypotheses(name)`` [K, d]) for the cost-table checks.
``solver_config(name)`` is the ``solver`` section the reference's classes and this package's are constructed with.  The sampler
draws from numpy's global RandomState, seeded with ``CASES[name]["init_seed"]`` just before ``estimate``.

The smallest shapes that reach each branch: 48 x 64 with patch 8 / slide 8 touches all four image borders with |p| up to 2.6
(integer shifts 0, +-1, +-2, -3: taps beyond the image); K = 67 is no multiple of 64; patch 5 / slide 3 overlaps, has odd boxes and
boxes cut by int(); 128 x 160 carries the boxes no LDS holds.
"""
import copy

import numpy as np

from _gml_cases import YAML_GML, frame_image, synth_events

P26 = {"min": -2.6, "max": 2.6}
V1 = {"min": -1.0, "max": 1.0}
ANGLE = {"min": 0, "max": 6.2832}
VEL_WARP = {"v_x": V1, "v_y": V1, "p_x": P26, "p_y": P26}
ANGLE_WARP = {"angle": ANGLE, "p_x": P26, "p_y": P26}               # configs/hot_plate1.yaml's parameterisation, wider p
VEL_ANGLEMAGN = {"v_x": V1, "v_y": V1, "p_angle": ANGLE, "p_magn": {"min": 0.0, "max": 2.6}}
VEL_ONLY = {"v_x": V1, "v_y": V1}
ANGLE_ONLY = {"angle": ANGLE}


def _case(kind, shape, roi, patch, slide, k, seed, params, sampler="random", gml=None, thresholding=False, thres=8, n_events=6000,
          clustered=False, special=False):
    g = dict(YAML_GML)
    g.update({"poisson_model": False, "weight_loss_by_inverse_event_hist": False, "angle_model": "angle" in params,
              "px-py_as-angle-magnitude": "p_angle" in params, "optimize_warp": any(q.startswith("p_") for q in params)})
    g.update(gml or {})
    return {"kind": kind, "shape": shape, "roi": roi, "k": k, "seed": seed, "init_seed": 3000 + seed, "gml": g, "params": params,
            "sampler": sampler, "n_events": n_events, "clustered": clustered, "special": special,
            "patch": {"patch_size": patch, "sliding_window": slide, "do_event_thresholding": thresholding, "event_thres": thres}}


S = (48, 64)
CASES = {
    "p8_k67": _case("patch", S, None, 8, 8, 67, 1, VEL_WARP, special=True),
    "p8_k1": _case("patch", S, None, 8, 8, 1, 2, VEL_WARP),
    "p5s3_we": _case("patch", S, (3, 45, 5, 60), 5, 3, 20, 3, VEL_WARP, gml={"weight_loss_by_event_hist": True}),
    "p5s3_inplace": _case("patch", S, (3, 45, 5, 60), 5, 3, 12, 4, VEL_WARP),   # overlap without weights: the reference's in-place division
    "nopol": _case("patch", S, None, 8, 8, 20, 5, VEL_WARP, gml={"no_polarity": True}),
    "angle": _case("patch", S, None, 8, 8, 20, 6, ANGLE_WARP, sampler="grid"),
    "anglemagn": _case("patch", S, None, 8, 8, 20, 7, VEL_ANGLEMAGN, sampler="uniform"),
    "nowarp": _case("patch", S, None, 8, 8, 20, 8, VEL_ONLY),
    "angle_grid1": _case("patch", S, None, 8, 8, 24, 9, ANGLE_ONLY, sampler="uniform"),   # one parameter: the whole grid, in order
    "thres": _case("patch", (64, 96), None, 8, 8, 20, 10, VEL_WARP, gml={"iwe_sigma": 0}, thresholding=True, thres=8, n_events=1500,
                   clustered=True),
    "global_roi": _case("global", S, (4, 44, 8, 60), None, None, 20, 11, VEL_WARP),
    "global_angle": _case("global", S, (4, 44, 8, 60), None, None, 20, 12, ANGLE_WARP),
    "global_full": _case("global", (128, 160), (0, 128, 0, 160), None, None, 10, 13, VEL_WARP, n_events=20000),
    # no LDS holds a 96 x 96 box: the ROI route (the patches overlap: event-hist weights keep the reference's histogram untouched)
    "p96_roi": _case("patch", (128, 160), None, 96, 32, 10, 14, VEL_WARP, gml={"weight_loss_by_event_hist": True}, n_events=20000),
}
ZERO_NORM_BOX = {"thres": (56, 64, 88, 96)}   # a box over the threshold whose polarity histogram is zero


def clustered_events(n, H, W, seed):
    """Events in three Gaussian blobs (integer pixels) that stay clear of the last patch row and column, and ten events in the
    bottom-right 8 x 8 box whose polarities cancel pixel by pixel: over the event threshold, with a zero histogram."""
    rs = np.random.RandomState(seed)
    centres = np.stack([rs.uniform(0.25 * H, 0.6 * H, 3), rs.uniform(0.25 * W, 0.6 * W, 3)], axis=1)
    which = rs.randint(0, 3, n)
    xy = centres[which] + rs.normal(0.0, 2.5, (n, 2))
    x = np.clip(np.round(xy[:, 0]), 0, H - 9)
    y = np.clip(np.round(xy[:, 1]), 0, W - 9)
    t = rs.uniform(0.0, 0.05, n)
    p = rs.randint(0, 2, n)
    ev = np.stack([x, y, t, p], axis=1).astype(np.float64)
    px = np.array([[H - 7, W - 6], [H - 5, W - 3], [H - 4, W - 7], [H - 2, W - 2], [H - 6, W - 4]], dtype=np.float64)
    pair = np.concatenate([np.concatenate([px, rs.uniform(0.0, 0.05, (5, 1)), np.full((5, 1), float(pol))], axis=1) for pol in (0, 1)])
    ev = np.concatenate([ev, pair])
    return ev[np.argsort(ev[:, 2], kind="stable")]


def case_inputs(name):
    """-> (frame [H, W] float64, events [n, 4] float64 (x = row, y = column, t, p))."""
    c = CASES[name]
    H, W = c["shape"]
    ev = (clustered_events if c["clustered"] else synth_events)(c["n_events"], H, W, 500 + c["seed"])
    return frame_image(H, W, 400 + c["seed"]), ev


def window_inputs(name, i):
    """Window i of a short recording over the case's geometry, for the batch tests."""
    c = CASES[name]
    H, W = c["shape"]
    return frame_image(H, W, 600 + 10 * c["seed"] + i), synth_events(c["n_events"], H, W, 700 + 10 * c["seed"] + i)


def roi_of(name):
    c = CASES[name]
    H, W = c["shape"]
    return c["roi"] if c["roi"] is not None else (0, H, 0, W)


def hypotheses(name):
    """The explicit table [K, d] of the case, in the order of ``CASES[name]["params"]``: seeded uniform draws in the ranges; the
    ``special`` case also carries fractions of exactly 0 and 31/32, the extreme shifts and an unwarped row."""
    c = CASES[name]
    rs = np.random.RandomState(800 + c["seed"])
    keys = list(c["params"])
    t = np.stack([rs.uniform(c["params"][k]["min"], c["params"][k]["max"], c["k"]) for k in keys], axis=1)
    if c["special"]:
        i, j = keys.index("p_x"), keys.index("p_y")
        rows = [(0.0, 0.0), (1.0, -2.0), (-31.0 / 32.0, 1.0 / 32.0), (2.6, -2.6), (-2.6, 2.6), (2.59, 2.6), (-2.6, -2.55), (0.5 / 32.0 + 1e-3, -1.0)]
        for r, (px, py) in enumerate(rows):
            t[r, i], t[r, j] = px, py
    return t


def solver_config(name, **optimizer_overrides):
    """The reference YAML's ``solver`` section for the case."""
    c = CASES[name]
    xmin, xmax, ymin, ymax = roi_of(name)
    opt = {"method": "optuna", "sampler": c["sampler"], "n_iter": c["k"], "parameters": copy.deepcopy(c["params"])}
    opt.update(optimizer_overrides)
    cfg = {
        "method": "patch_eklt" if c["kind"] == "patch" else "generative_max_likelihood",
        "filter": {"filters": [], "parameters": {"xmin": xmin, "xmax": xmax, "ymin": ymin, "ymax": ymax}},
        "warp_direction": "first", "motion_model": "2d-translation", "parameters": ["trans_x", "trans_y"], "cost": "hybrid",
        "outer_padding": 0, "cost_with_weight": {"diff_norm": 1.0},
        "iwe": {"method": "bilinear_vote", "blur_sigma": 3},
        "optimizer": opt,
        "generative_ml": copy.deepcopy(c["gml"]),
    }
    if c["kind"] == "patch":
        cfg["patch_eklt"] = dict(c["patch"])
    return cfg


def stored_rows(name):
    """The rows of the output flow the fixture keeps: every 6th at 48 and 64 rows, every 32nd at 128."""
    H = CASES[name]["shape"][0]
    return np.arange(0, H, 32 if H >= 128 else 6)
