"""Plain numpy restatement of the reference's sampled EKLT solvers: ``PatchEklt`` (src/solver/patch_eklt.py) and
``GenerativeMaximumLikelihood`` (src/solver/generative_max_likelihood.py) on their numpy route -- the objective
(``_make_prediction_numpy``, ``_make_measured_increment``, diff_norm), ``unfold_params``, the sampler tables and ``estimate``.

It is the CPU checker of the HIP sweep (tests/test_gpu_eklt.py) and is itself pinned to the reference by
tests/golden/golden_eklt.npz (tests/test_eklt.py).  The measurement planes (Sobel of the model image, blurred histogram, weights)
are tests/_gml_ref.py's ``prepare``; the warp is tests/_eklt_warp64.py's.

Where this package departs from the reference, this module follows the package unless told otherwise:
* ``inplace=True`` restates ``PatchEklt._make_measured_increment``'s division of a VIEW of the cached histogram (no event-hist
  weights): patches are visited in order and each divides its box of the shared histogram in place, so an overlapping later patch
  sees the earlier divisions.  The default normalises the untouched histogram.
* a box whose histogram norm is 0 is not evaluated (the reference divides by zero).
* one hypothesis table per ``estimate`` call, shared by all patches (the reference opens an optuna study per patch).
"""
import numpy as np
import torch

import _gml_dep_ref as D
import _gml_ref as R
from _eklt_warp64 import translation, warp_perspective_f64


# ------------------------------------------------------------------ parameters
def unfold(gml, keys, table):
    """unfold_params over a table [K, d] whose columns are ``keys`` -> [K, 4]: v_x, v_y, p_x, p_y (p = 0 without optimize_warp)."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, len(keys))
    col = {k: t[:, i] for i, k in enumerate(keys)}
    out = np.zeros((t.shape[0], 4))
    if gml.get("angle_model"):
        out[:, 0], out[:, 1] = np.sin(col["angle"]), np.cos(col["angle"])
    else:
        out[:, 0], out[:, 1] = col["v_x"], col["v_y"]
    if gml.get("optimize_warp"):
        if gml.get("px-py_as-angle-magnitude"):
            out[:, 2], out[:, 3] = col["p_magn"] * np.sin(col["p_angle"]), col["p_magn"] * np.cos(col["p_angle"])
        else:
            out[:, 2], out[:, 3] = col["p_x"], col["p_y"]
    return out


def sampler_table(opt):
    """The hypothesis table [n_iter, d] of an ``optimizer`` section, drawn from numpy's global RandomState."""
    keys = list(opt["parameters"])
    n = int(opt["n_iter"])
    lo = np.array([opt["parameters"][k]["min"] for k in keys], dtype=np.float64)
    hi = np.array([opt["parameters"][k]["max"] for k in keys], dtype=np.float64)
    if opt["sampler"] == "random":
        return np.array([[np.random.uniform(lo[j], hi[j]) for j in range(len(keys))] for _ in range(n)]).reshape(n, len(keys))
    assert opt["sampler"] in ("uniform", "grid")
    axes = [np.arange(lo[j], hi[j], (hi[j] - lo[j]) / n) for j in range(len(keys))]
    if len(keys) == 1:
        return axes[0].reshape(-1, 1).astype(np.float64)
    return np.array([[axes[j][np.random.randint(len(axes[j]))] for j in range(len(keys))] for _ in range(n)], dtype=np.float64)


# ------------------------------------------------------------------ geometry
def patch_boxes(H, W, p, s):
    """prepare_patch + FlowPatch bounds as numpy slices them -> [gh gw, 4] int: rows [r0, r1), columns [c0, c1), row-major over the
    patch grid."""
    cx, cy = D.axis(H, p, s)[0], D.axis(W, p, s)[0]
    lo = lambda c: int(c - np.ceil(p / 2))
    hi = lambda c: int(c + np.floor(p / 2))
    return np.array([[lo(a), min(hi(a), H), lo(b), min(hi(b), W)] for a in cx for b in cy], dtype=np.int64)   # (slices end at the edge)


# ------------------------------------------------------------------ the objective
def warped_gradients(st, px, py, warp):
    if not warp:
        return st["gx"], st["gy"]
    H, W = st["gx"].shape
    M = translation(px, py)
    return warp_perspective_f64(st["gx"], M, (W, H)), warp_perspective_f64(st["gy"], M, (W, H))


def measured(st, box, hist=None):
    """_make_measured_increment on a box -> (Q, weights or None); Q is None where the box's norm is 0 or not finite."""
    r0, r1, c0, c1 = box
    h = st["hist"] if hist is None else hist
    m = h[r0:r1, c0:c1]
    we = None
    if st["we"] is not None:
        we = st["we"][r0:r1, c0:c1]
        m = we * m
    n = np.linalg.norm(m)
    if not n > 0:
        return None, we
    if hist is not None and st["we"] is None:
        m /= n          # the reference: a view of the cache, divided in place
        return m, we
    return m / n, we


def predicted(st, gml, box, hyp, we, cache=None):
    """_make_prediction_numpy -> P."""
    r0, r1, c0, c1 = box
    vx, vy, px, py = (float(v) for v in hyp)
    key = (px, py)
    if cache is not None and key in cache:
        Gx, Gy = cache[key]
    else:
        Gx, Gy = warped_gradients(st, px, py, gml.get("optimize_warp"))
        if cache is not None:
            cache[key] = (Gx, Gy)
    P = vx * Gx[r0:r1, c0:c1] + vy * Gy[r0:r1, c0:c1]
    if gml.get("no_polarity"):
        P = np.abs(P)
    if we is not None:
        P *= we
    P /= np.linalg.norm(P) + 0.0001
    return P


def cost_and_bar(P, Q, w):
    """-> (w max_c sum_r |Q - P|, the forward-error bound of one column sum summed in any order, times w: n_box 2^-52 times the
    largest column's sum |P| + sum |Q|)."""
    cost = w * np.linalg.norm(Q - P, ord=1)
    bar = abs(w) * P.size * 2.0 ** -52 * float((np.abs(P).sum(0) + np.abs(Q).sum(0)).max())
    return cost, bar


def column_margin(P, Q):
    """(largest - second largest) / largest column sum of |Q - P| (1 for a single column)."""
    cs = np.sort(np.abs(Q - P).sum(0))[::-1]
    return 1.0 if len(cs) < 2 else float((cs[0] - cs[1]) / cs[0])


def cost_table(st, gml, boxes, hyp4, w, selected=None, inplace=False, want_bar=False):
    """-> cost [P, K] (NaN rows where a box is unselected or has a zero norm), evaluated [P] bool, and (``want_bar``) bar [P, K]."""
    hyp4 = np.asarray(hyp4, dtype=np.float64).reshape(-1, 4)
    Pn, K = len(boxes), len(hyp4)
    cost, bar, ok = np.full((Pn, K), np.nan), np.full((Pn, K), np.nan), np.zeros(Pn, dtype=bool)
    hist = st["hist"].copy() if inplace else None
    cache = {}
    for i, box in enumerate(boxes):
        if selected is not None and not selected[i]:
            continue
        Q, we = measured(st, box, hist)
        if Q is None:
            continue
        ok[i] = True
        for k in range(K):
            cost[i, k], bar[i, k] = cost_and_bar(predicted(st, gml, box, hyp4[k], we, cache), Q, w)
    return (cost, ok, bar) if want_bar else (cost, ok)


def argmin_rows(cost):
    """The row argmin, the lowest index on a tie, NaN never winning; -1 where a row has no number."""
    c = np.where(np.isnan(cost), np.inf, cost)
    idx = np.argmin(c, axis=1)
    return np.where(np.isfinite(c[np.arange(len(c)), idx]), idx, -1)


# ------------------------------------------------------------------ estimate
def state(frame, events, gml, roi):
    H, W = np.shape(frame)
    return R.prepare(frame, R.polarity_image(events, (H, W)), gml, roi)


def estimate_patch(frame, events, cfg, inplace=False):
    """PatchEklt.estimate with one table per call -> (flow [2, H, W], selected [P] bool, best index [P], cost [P, K], hyp4)."""
    gml, pe, opt = cfg["generative_ml"], cfg["patch_eklt"], cfg["optimizer"]
    H, W = np.shape(frame)
    fp = cfg["filter"]["parameters"]
    roi = (fp["xmin"], fp["xmax"], fp["ymin"], fp["ymax"])
    p, s = pe["patch_size"], pe.get("sliding_window", pe["patch_size"])
    st = state(frame, events, gml, roi)
    boxes = patch_boxes(H, W, p, s)
    sel = np.zeros(len(boxes), dtype=bool)
    sel[D.select(events, H, W, p, s, roi, pe["do_event_thresholding"], pe.get("event_thres"))] = True
    hyp4 = unfold(gml, list(opt["parameters"]), sampler_table(opt))
    cost, ok = cost_table(st, gml, boxes, hyp4, cfg["cost_with_weight"]["diff_norm"], sel, inplace)
    best = argmin_rows(cost)
    gh, gw = D.grid_shape(H, W, p, s)
    grid = np.zeros((2, gh * gw))
    won = best >= 0
    grid[:, won] = hyp4[best[won], :2].T
    flow = D.upsample(torch.from_numpy(grid.reshape(2, gh, gw)), p, s, H, W).numpy()
    return flow, ok, best, cost, hyp4


def estimate_global(frame, events, cfg):
    """GenerativeMaximumLikelihood.estimate -> (flow [2, H, W], evaluated [1], best index [1], cost [1, K], hyp4)."""
    gml, opt = cfg["generative_ml"], cfg["optimizer"]
    H, W = np.shape(frame)
    fp = cfg["filter"]["parameters"]
    roi = (fp["xmin"], fp["xmax"], fp["ymin"], fp["ymax"])
    st = state(frame, events, gml, roi)
    hyp4 = unfold(gml, list(opt["parameters"]), sampler_table(opt))
    cost, ok = cost_table(st, gml, np.array([roi]), hyp4, cfg["cost_with_weight"]["diff_norm"])
    best = argmin_rows(cost)
    flow = np.zeros((2, H, W))
    if best[0] >= 0:
        flow[0], flow[1] = hyp4[best[0], 0], hyp4[best[0], 1]
    return flow, ok, best, cost, hyp4
