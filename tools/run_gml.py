#!/usr/bin/env python3
"""End-to-end run of the generative BOS solver (solver.GenerativePatchPyramid, the reference's patch_eklt_pyramid2) on a synthetic
BOS scene with a known displacement field.

    python tools/run_gml.py                                                   # 260 x 346, the reference YAML's options
    python tools/run_gml.py --size 128 160 --n_iter 120 --json out.json
    python tools/run_gml.py --config_file tests/golden/config_hot_plate1.json # the REFERENCE's configs/hot_plate1.yaml, as it is
    python tools/run_gml.py --method patch_eklt_dependent                     # the single-scale solver, the YAML's patch_eklt block
    python tools/run_gml.py --method patch_eklt --n_iter 800                  # the sampled solvers: n_iter hypotheses per patch
    python tools/run_gml.py --method generative_max_likelihood --n_iter 800   #   ... or for the one ROI (solver/eklt_sweep.py)
    python tools/run_gml.py --batch 8                                         # 8 windows of the scene through estimate_batch

The scene: a textured frame L, a potential phi (two Gaussian bumps) and its gradient d = grad phi as the displacement; events are
drawn at pixels with probability proportional to |grad L . d|, with the sign of grad L . d as polarity.  Reported: the loss at
the first and the last Adam iteration, the time per scale and per window, and EPE / AE (event_based_bos_amd.flow_error) and the
cosine between the recovered flow and d inside the ROI.  The generative model normalises its prediction, so the flow's scale
is free: the cosine is the meaningful figure, EPE is shown for completeness.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(H, W, n_events, seed=0):
    rs = np.random.RandomState(seed)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    frame = 128 + 60 * np.sin(2 * np.pi * r / 19.0) * np.cos(2 * np.pi * c / 27.0) + 20 * np.sin(2 * np.pi * (r + c) / 41.0)
    phi = np.zeros((H, W))
    for cy, cx, s, a in ((0.45, 0.4, 0.18, 40.0), (0.6, 0.65, 0.12, -25.0)):
        phi += a * np.exp(-((r - cy * H) ** 2 + (c - cx * W) ** 2) / (2 * (s * min(H, W)) ** 2))
    d = np.stack(np.gradient(phi))                     # [2, H, W]: d / d row, d / d column
    g = np.stack(np.gradient(frame))
    inc = g[0] * d[0] + g[1] * d[1]
    prob = np.abs(inc).ravel() / np.abs(inc).sum()
    idx = rs.choice(H * W, size=n_events, p=prob)
    ev = np.stack([idx // W, idx % W, np.sort(rs.uniform(0, 0.05, n_events)), (inc.ravel()[idx] > 0)], axis=1).astype(np.float64)
    return frame, ev, d


SWEEPS = ("patch_eklt", "generative_max_likelihood")


def default_config(H, W, n_iter, method="patch_eklt_pyramid2"):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _gml_cases import YAML_COST, YAML_GML
    cfg = {"method": method, "filter": {"filters": [], "parameters": {"xmin": 0, "xmax": H, "ymin": 0, "ymax": W}},
           "cost_with_weight": dict(YAML_COST), "optimizer": {"method": "Adam", "n_iter": n_iter}, "generative_ml": dict(YAML_GML)}
    if method in SWEEPS:   # the reference YAML's optuna block: the angle model, a translation within 0.4 px
        cfg["cost_with_weight"] = {"diff_norm": 1.0}
        cfg["optimizer"] = {"method": "optuna", "sampler": "random", "n_iter": n_iter,
                            "parameters": {"angle": {"min": 0, "max": 6.2832}, "p_x": {"min": -0.4, "max": 0.4}, "p_y": {"min": -0.4, "max": 0.4}}}
        cfg["generative_ml"].update({"angle_model": True, "poisson_model": False})
    if method in ("patch_eklt_dependent", "patch_eklt"):
        cfg["patch_eklt"] = {"patch_size": 4, "sliding_window": 2, "do_event_thresholding": False, "event_thres": 8}
    return cfg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=(260, 346), metavar=("H", "W"))
    ap.add_argument("--n_iter", type=int, default=600)
    ap.add_argument("--events", type=int, default=0, help="events in the window (default 2 per pixel)")
    ap.add_argument("--config_file", default=None, help="a reference config (JSON with a 'propagated' section, or a solver dict)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--method", default="patch_eklt_pyramid2", choices=("patch_eklt_pyramid2", "patch_eklt_dependent") + SWEEPS,
                    help="the solver when no --config_file is given")
    ap.add_argument("--batch", type=int, default=0, metavar="B",
                    help="also solve B windows of the scene (different event seeds and counts) with estimate_batch: per-window time "
                         "beside the sequential window's, and whether window 0 equals the sequential result bit for bit")
    ap.add_argument("--json", default=None, help="also write the result here")
    args = ap.parse_args()

    import event_based_bos_amd as ebos
    from event_based_bos_amd.flow_error import calculate_flow_error_numpy

    if args.config_file:
        with open(args.config_file) as f:
            cfg = json.load(f)
        cfg = cfg.get("propagated", cfg)
        H, W = int(cfg["data"]["height"]), int(cfg["data"]["width"])
        solver_cfg = cfg["solver"]
    else:
        H, W = args.size
        solver_cfg = default_config(H, W, args.n_iter, args.method)
    method = solver_cfg["method"]
    frame, events, d = scene(H, W, args.events or 2 * H * W, args.seed)
    import types
    reg = types.SimpleNamespace(SolverBase=ebos.solver.SolverBase, collections={})
    ebos.solver.register_generative_into(reg)          # method patch_eklt_pyramid2, no override
    ebos.solver.register_dependent_into(reg)           # method patch_eklt_dependent
    ebos.solver.register_eklt_into(reg)                # methods patch_eklt, generative_max_likelihood
    solv = reg.collections[method]((H, W), (H, W), {}, solver_cfg)
    np.random.seed(args.seed)
    solv.estimate(events, frame=frame, background=frame)   # warm-up (code objects, allocations)
    import torch
    torch.cuda.synchronize()
    np.random.seed(args.seed)
    t0 = time.perf_counter()
    flow = solv.estimate(events, frame=frame, background=frame)
    t_window = time.perf_counter() - t0
    h = solv.cost_func.get_history()
    xmin, xmax, ymin, ymax = solv._gml_roi
    m = np.zeros((H, W), dtype=bool)
    m[xmin:xmax, ymin:ymax] = True
    fr, dr = flow[:, m], d[:, m]
    cos = float((fr * dr).sum() / (np.linalg.norm(fr) * np.linalg.norm(dr) + 1e-300))
    err = calculate_flow_error_numpy(d[None], flow[None], m[None, None].astype(np.float64))
    n_it = len(h["loss"])
    res = {"method": method, "size": [H, W], "roi": [xmin, xmax, ymin, ymax], "iterations": n_it, "events": int(len(events)),
           "loss_first": float(h["loss"][0]) if n_it else None, "loss_last": float(h["loss"][-1]) if n_it else None,
           "window_ms": 1e3 * t_window,
           "ms_per_iteration": 1e3 * t_window / max(n_it, 1), "cosine_roi": cos,
           "EPE": float(err["EPE"]), "AE": float(err["AE"])}
    if args.batch > 0:
        n_ev = args.events or 2 * H * W
        windows = [events] + [scene(H, W, n_ev - (i % 4) * (n_ev // 8), args.seed + i)[1] for i in range(1, args.batch)]
        np.random.seed(args.seed)
        solv.estimate_batch(windows, frames=frame, background=frame)   # warm-up
        torch.cuda.synchronize()
        np.random.seed(args.seed)
        t0 = time.perf_counter()
        flows = solv.estimate_batch(windows, frames=frame, background=frame)
        t_batch = time.perf_counter() - t0
        res.update({"batch": args.batch, "batch_window_ms": 1e3 * t_batch / args.batch,
                    "batch_ms_per_iteration": 1e3 * t_batch / args.batch / max(n_it, 1),
                    "batch_vs_sequential": t_window / (t_batch / args.batch),
                    "batch_window0_bit_identical": bool(np.array_equal(flows[0], flow))})
    if method in SWEEPS:   # no iterations: hypotheses, and the winners' costs
        sel = solv.estimate_indices
        res.update({"hypotheses": int(solver_cfg["optimizer"]["n_iter"]), "boxes": int(solv.n_patch), "boxes_scored": int(len(sel)),
                    "best_value_mean": float(np.mean(solv.best_values[sel])) if len(sel) else None})
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
