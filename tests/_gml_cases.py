"""Seeded cases of the generative patch-pyramid solver (tests/golden/golden_gml.npz; tests/test_gml.py, tests/test_gpu_gml.py).

A case is a window of synthetic events over a textured frame, a ROI, the reference's ``generative_ml`` options and ``n_iter``.
``case_inputs(name)`` rebuilds the frame and the events from seeds; ``solver_config(name)`` is the ``solver`` section the
reference's ``PatchEkltPyramid2`` and this package's ``GenerativePatchPyramid`` are constructed with.  The initial potentials are
drawn from numpy's global RandomState, seeded with ``CASES[name]["init_seed"]`` just before ``estimate``.
"""
import copy

import numpy as np

YAML_GML = {   # configs/hot_plate1.yaml of the reference, solver.generative_ml
    "weight_loss_by_event_hist": False, "weight_sigma": 5, "weight_loss_by_inverse_event_hist": True, "optimize_warp": True,
    "iwe_sigma": 2, "viz_diff_scale": [-0.25, 0.25], "no_polarity": False, "model_image": "current", "use_log_intensity": False,
    "poisson_model": True,
}
YAML_COST = {"diff_norm": 1.0, "image_gradient": 0.5, "flow_norm_pxy": 0.1}


def _case(shape, roi, n_iter, n_events, seed, gml=None, cost=None):
    g = dict(YAML_GML)
    g.update(gml or {})
    return {"shape": shape, "roi": roi, "n_iter": n_iter, "n_events": n_events, "seed": seed, "init_seed": 1000 + seed,
            "gml": g, "cost": dict(cost or YAML_COST)}


CASES = {
    "yaml_128": _case((128, 160), None, 600, 20000, 1),
    "yaml_128_roi": _case((128, 160), (16, 112, 32, 120), 120, 20000, 2),
    "nowarp_128": _case((128, 160), (8, 120, 0, 160), 120, 20000, 3, {"optimize_warp": False},
                        {"diff_norm": 1.0, "image_gradient": 0.5}),
    "nopol_128": _case((128, 160), (16, 112, 32, 120), 120, 20000, 4, {"no_polarity": True}),
    "evhist_128": _case((128, 160), (16, 112, 32, 120), 120, 20000, 5, {"weight_loss_by_event_hist": True}),
    "sigma0_log_128": _case((128, 160), None, 120, 20000, 6, {"iwe_sigma": 0, "use_log_intensity": True,
                                                              "weight_loss_by_inverse_event_hist": False}),
    "yaml_260": _case((260, 346), (0, 260, 86, 260), 120, 60000, 7),
    "terms_260": _case((260, 346), None, 120, 60000, 8, None, {"flow_norm_pxy": 0.2, "diff_norm": 2.0}),
    "yaml_720": _case((720, 1280), (0, 720, 320, 960), 8, 400000, 9),
}


def frame_image(H, W, seed):
    """A textured float64 frame in [0, 255]: two sinusoids and seeded noise."""
    rs = np.random.RandomState(seed)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = rs.uniform(0, 2 * np.pi, 2)
    f = 128.0 + 50.0 * np.sin(2 * np.pi * r / 23.0 + ph[0]) * np.cos(2 * np.pi * c / 31.0 + ph[1]) + rs.normal(0.0, 12.0, (H, W))
    return np.clip(f, 0.0, 255.0)


def synth_events(n, H, W, seed):
    rs = np.random.RandomState(seed)
    x = rs.randint(0, H, n)
    y = rs.randint(0, W, n)
    t = np.sort(rs.uniform(0.0, 0.05, n))
    p = rs.randint(0, 2, n)
    return np.stack([x, y, t, p], axis=1).astype(np.float64)


def case_inputs(name):
    """-> (frame [H, W] float64, events [n, 4] float64 (x = row, y = column, t, p))."""
    c = CASES[name]
    H, W = c["shape"]
    return frame_image(H, W, 100 + c["seed"]), synth_events(c["n_events"], H, W, 200 + c["seed"])


def roi_of(name):
    c = CASES[name]
    H, W = c["shape"]
    return c["roi"] if c["roi"] is not None else (0, H, 0, W)


def solver_config(name, **gml_overrides):
    """The reference YAML's ``solver`` section for the case (method patch_eklt_pyramid2)."""
    c = CASES[name]
    xmin, xmax, ymin, ymax = roi_of(name)
    g = copy.deepcopy(c["gml"])
    g.update(gml_overrides)
    return {
        "method": "patch_eklt_pyramid2",
        "filter": {"filters": [], "parameters": {"xmin": xmin, "xmax": xmax, "ymin": ymin, "ymax": ymax}},
        "warp_direction": "first", "motion_model": "2d-translation", "parameters": ["trans_x", "trans_y"], "cost": "hybrid",
        "outer_padding": 0, "cost_with_weight": dict(c["cost"]),
        "iwe": {"method": "bilinear_vote", "blur_sigma": 3},
        "optimizer": {"method": "Adam", "n_iter": c["n_iter"],
                      "parameters": {"angle": {"min": 0, "max": 6.2832}, "p_x": {"min": -0.4, "max": 0.4},
                                     "p_y": {"min": -0.4, "max": 0.4}}},
        "generative_ml": g,
        "patch_eklt": {"patch_size": 4, "sliding_window": 2, "do_event_thresholding": False, "event_thres": 8},
    }


def stored_rows(name):
    """The rows of the output flow the fixture keeps (with max|flow|): every 16th at 128 x 160, every 32nd at 260 x 346, every
    192nd at 720 x 1280.  float64 flows do not compress, and the fixture stays small."""
    H = CASES[name]["shape"][0]
    return np.arange(0, H, 192 if H >= 720 else (32 if H >= 260 else 16))


def stored_param_rows(name, scale):
    """None: the whole parameter grid of a scale is stored; else its grid rows kept (720 x 1280: every 3rd of the 45 rows at
    scale 3, every 18th of the 90 rows at scale 4)."""
    if CASES[name]["shape"][0] >= 720 and scale == 3:
        return np.arange(0, 45, 3)
    if CASES[name]["shape"][0] >= 720 and scale == 4:
        return np.arange(0, 90, 18)
    return None
