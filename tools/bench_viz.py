#!/usr/bin/env python3
"""Timing of the visualizer's pictures (event_based_bos_amd/visualizer.py, csrc/visualize.hip).

    python tools/bench_viz.py [--out profiles/viz_bench.json] [--rounds 5] [--reps 30] [--no-host] [--no-eval]

Per window at 260 x 346 and 720 x 1280, B = 1 and 8:

(a) the ten pictures of a driver step on the device (``render_step_batch``), split into the render side (mask close, reduce, ten
    render launches) and the Poisson integration of the two flows.  Times are device events around a loop of calls, taken in
    alternating rounds (render, Poisson, whole step, render, ...); the median over the rounds and their spread (min, max) are kept.
(b) for the render side alone: the bytes it must move (every input plane read once per picture that needs it, every picture written
    once) over its time, as a share of the device-to-device copy rate measured in the same run (a 256 MiB copy).
(c) the host: the same ten pictures through the numpy restatement (tests/_viz_ref.py) with the host Poisson restatement
    (tests/_poisson_ref.py), one window.
(d) ``RecordingEvaluator`` per step with ``pictures=True`` against ``pictures=False`` in the same process, alternating, on the
    synthetic recording of ``tools/run_eval.py`` (its pictures include the read-back and the PNG encoding on the host).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import event_based_bos_amd as ebos  # noqa: E402
from event_based_bos_amd import _hip, visualizer as V  # noqa: E402
from event_based_bos_amd.poisson import poisson_reconstruct_batch  # noqa: E402

SHAPES = [(260, 346), (720, 1280)]
BATCHES = [1, 8]


def inputs(shape, B, seed=0):
    rs = np.random.RandomState(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    pred = np.stack([np.stack([2.5 * np.sin(yy / 37.0 + b), 1.5 * np.cos(xx / 41.0)]) + 0.3 * rs.randn(2, H, W) for b in range(B)])
    gt = np.stack([np.stack([2.0 * np.sin(yy / 31.0), 3.0 * np.cos(xx / 43.0 + b)]) + 0.2 * rs.randn(2, H, W) for b in range(B)])
    oc = rs.poisson(0.3, (B, 2, H, W)).astype(np.float64)
    fc = oc * (rs.rand(B, 1, H, W) < 0.6)
    return pred, gt, (fc.sum(1) != 0).astype(np.uint8), fc, oc


def event_time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def copy_rate():
    a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    return 2 * a.numel() / event_time(lambda: b.copy_(a), 20)


def render_bytes(shape, pad=0):
    """Bytes per window the render side must move: reads of the planes each launch needs, writes of every picture."""
    n = shape[0] * shape[1]
    flow, plane, mask, rgb, grey = 16 * n, 8 * n, n, 3 * n, n
    close = 2 * mask
    reduce_ = 2 * flow + flow + flow + (flow + mask) + (flow + mask) + 2 * plane
    render = 2 * plane + grey + 2 * plane + grey + 4 * (flow + rgb) + 2 * (flow + mask + rgb) + 2 * (plane + grey)
    return close + reduce_ + render


def render_only(pred, gt, mask, fc, oc, p_pred, p_gt, ord=0.5):
    """The render side of ``render_step_batch`` on Poisson fields integrated before: the same launches, in the same order."""
    closed = V.mask_close(mask)
    s = V.reduce_scales([V._flow_field(pred, pair=gt), V._flow_field(pred), V._flow_field(gt), V._flow_field(pred, mask=closed),
                         V._flow_field(gt, mask=closed), V._scalar_field(p_pred), V._scalar_field(p_gt)], ord)
    on_mask = _hip.VIZ_MASK_MULTIPLY | _hip.VIZ_MASK_BLACK
    return (V.event_picture(oc), V.clipped_iwe_picture(fc[:, 0], 50, 0, second=fc[:, 1]), V.flow_rgb(pred, s[:, 0], ord=ord),
            V.flow_rgb(gt, s[:, 0], ord=ord), V.flow_rgb(pred, s[:, 1], ord=ord), V.centered_picture(p_pred, s[:, 5]),
            V.flow_rgb(pred, s[:, 3], closed, on_mask, ord), V.flow_rgb(gt, s[:, 2], ord=ord), V.centered_picture(p_gt, s[:, 6]),
            V.flow_rgb(gt, s[:, 4], closed, on_mask, ord))


def stats(values):
    v = np.array(values)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def device_rows(rounds, reps, rate):
    rows = []
    for shape in SHAPES:
        for B in BATCHES:
            pred, gt, mask, fc, oc = (torch.from_numpy(a).cuda() for a in inputs(shape, B))
            both = poisson_reconstruct_batch(torch.cat([pred, gt]))
            p_pred, p_gt = both[:B].contiguous(), both[B:].contiguous()
            calls = {"render": lambda: render_only(pred, gt, mask, fc, oc, p_pred, p_gt),
                     "poisson": lambda: poisson_reconstruct_batch(torch.cat([pred, gt])),
                     "step": lambda: V.render_step_batch(pred, gt, mask, fc, oc)}
            times = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    times[k].append(event_time(fn, reps) / B * 1e6)
            nbytes = render_bytes(shape)
            t_render = np.median(times["render"]) * 1e-6
            rows.append({"shape": list(shape), "B": B, "us_per_window": {k: stats(v) for k, v in times.items()},
                         "render_bytes_per_window": nbytes, "render_GB_per_s": nbytes / t_render / 1e9,
                         "render_share_of_measured_copy_rate": nbytes / t_render / rate})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def host_rows():
    import _poisson_ref as P
    import _viz_ref as R

    rows = []
    for shape in SHAPES:
        pred, gt, mask, fc, oc = (a[0] for a in inputs(shape, 1))
        H, W = shape
        rs = np.random.RandomState(1)
        orig = np.stack([rs.randint(0, H, 20000), rs.randint(0, W, 20000), np.zeros(20000), rs.randint(0, 2, 20000)], axis=1).astype(np.float64)
        t0 = time.perf_counter()
        fields = [P.restated_poisson(f[1], f[0], np.zeros(shape)) for f in (pred, gt)]
        t1 = time.perf_counter()
        R.step_pictures(orig, orig[::2], pred, gt, shape, fields[0], fields[1])
        t2 = time.perf_counter()
        rows.append({"shape": list(shape), "poisson_ms_per_window": (t1 - t0) * 1e3, "pictures_ms_per_window": (t2 - t1) * 1e3})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def eval_rows(rounds):
    import run_eval
    from event_based_bos_amd.evaluation import RecordingEvaluator, synthetic_recording

    tmp = tempfile.mkdtemp(prefix="ebos_viz_bench_")
    shape, roi = (128, 160), (0, 128, 16, 144)
    ev_path, fr_path, tr_path, stamps = synthetic_recording(os.path.join(tmp, "rec"), shape, 12, 8000)
    cfg = ebos.utils.propagate_config(run_eval.synthetic_config(shape, roi, stamps, 20))
    events, frames = ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path)
    times = {False: [], True: []}
    for r in range(rounds + 1):
        for pictures in (False, True):
            solv = run_eval.build_solver(ebos, cfg)
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = RecordingEvaluator(cfg, events, frames, solv, save_dir=os.path.join(tmp, f"o{r}{int(pictures)}")).run(8, pictures=pictures)
            torch.cuda.synchronize()
            if r:      # (round 0 warms up)
                times[pictures].append((time.perf_counter() - t0) / len(res.steps) * 1e3)
    row = {"shape": list(shape), "steps": len(res.steps), "ms_per_step_pictures_off": stats(times[False]),
           "ms_per_step_pictures_on": stats(times[True]),
           "note": "host clock around run() ending in a synchronise; pictures on includes the read-back and the PNG encoding of ten files per step"}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viz_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_viz needs a GPU"
    rate = copy_rate()
    res = {"device": torch.cuda.get_device_name(0), "measured_copy_rate_GB_per_s": rate / 1e9, "rounds": args.rounds, "reps": args.reps}
    print(json.dumps(res), flush=True)
    res["device_step"] = device_rows(args.rounds, args.reps, rate)
    if not args.no_host:
        res["host_restatement"] = host_rows()
    if not args.no_eval:
        res["evaluator"] = eval_rows(min(args.rounds, 3))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
