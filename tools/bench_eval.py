#!/usr/bin/env python
"""Time the recording evaluator against the sequential loop over the existing public calls, in one process.

    python tools/bench_eval.py [--shapes 260,720] [--solvers pyramid,dependent] [--max-batch 1,4,8] [--n-iter 600] [--repeats 5]
                               [--out profiles/eval_bench.json] [--ingest-only]

Both sides evaluate the same synthetic recording (about 100 k events per window at 260 x 346; the YAML's ROI at 720 x 1280).  The
sides do the same work (both write the three text files) and alternate, after one warm-up each; the library's launch profiler
(``ebos_profile_start``) is never started and no torch profiler is used; the best and the spread (max - min) of each side are reported per step, and the raw
times are written as JSON.  ``--ingest-only`` runs only the window ingest and the path it replaces (upload + polarity splat +
event mask + period) a few times: the run to put under ``rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py --ingest-only``.

``--solvers cmax_time_aware``: the time-aware contrast maximisation as a native loop (configs/cmax_time_aware_eval.yaml's solver
section, patch sized to the geometry).  Its two sides are the evaluator with the solver's ``estimate_batch_prepared`` (stacked plans
from the raw columns, the batch loop) and the same evaluator with that method hidden, i.e. the window-by-window ``preprocess`` +
``estimate`` route; both are timed with device events, best and [min, max] of alternating rounds.
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import run_eval  # noqa: E402

GEOMETRY = {260: ((260, 346), (0, 260, 86, 260), 100_000), 720: ((720, 1280), (0, 720, 320, 960), 400_000)}
METHOD = {"pyramid": "patch_eklt_pyramid2", "dependent": "patch_eklt_dependent"}


def sequential_loop(ebos, cfg, events, frames, solv, save_dir):
    """The driver's loop over the existing public calls, one window at a time (what the evaluator replaces)."""
    from event_based_bos_amd.evaluation import TEXT_TIMESTAMPS, TEXT_WITH_MASK, TEXT_WITHOUT_MASK, plan_evaluation, save_line
    from event_based_bos_amd.frame_flow import FrameFlowEstimator

    common = cfg["common_params"]
    est = FrameFlowEstimator(None)
    im0, _ = frames.load_image(0)
    frame0 = ebos.validate_image(im0, common)
    roi = (slice(None), slice(common["xmin"], common["xmax"]), slice(common["ymin"], common["ymax"]))
    out = []
    for s in plan_evaluation(cfg, events, frames):
        im1, _ = frames.load_image(s.i1)
        im2, _ = frames.load_image(s.i2)
        gt = est.estimate(cfg["method"], frame0, ebos.validate_image(im1, common), ebos.validate_image(im2, common), cfg)
        filtered, _ = solv.preprocess(events.load_event(*s.est_range))
        flow = solv.estimate(filtered, gt, frame=im1, background=im0)
        e0 = solv.calculate_flow_error(flow[roi], gt[roi])
        e1 = solv.calculate_flow_error(flow[roi], gt[roi], events=filtered, roi=common)
        save_line(solv, s.i_frame, e0, TEXT_WITHOUT_MASK, save_dir)   # (the same three lines the evaluator writes)
        save_line(solv, s.i_frame, e1, TEXT_WITH_MASK, save_dir)
        save_line(solv, s.i_frame, {"t1": s.t1, "t2": s.t2}, TEXT_TIMESTAMPS, save_dir)
        out.append((e0, e1))
    return out


def bench_case(ebos, size, kind, max_batches, n_iter, repeats, n_frames):
    import torch
    from event_based_bos_amd.evaluation import RecordingEvaluator, synthetic_recording

    shape, roi, per = GEOMETRY[size]
    tmp = tempfile.mkdtemp(prefix="ebos_bench_eval_")
    ev_path, fr_path, tr_path, stamps = synthetic_recording(tmp, shape, n_frames, per)
    cfg = run_eval.synthetic_config(shape, roi, stamps, n_iter)
    cfg["solver"]["method"] = METHOD[kind]
    cfg = ebos.utils.propagate_config(cfg)
    events, frames = ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path)
    os.chdir(tmp)   # (the solver's text writer appends to the working directory)
    rows = []
    for mb in max_batches:
        times = {"loop": [], "evaluator": []}
        n_steps = None
        for rep in range(repeats + 1):   # (rep 0 warms both sides up)
            for side in ("loop", "evaluator"):
                solv = run_eval.build_solver(ebos, copy.deepcopy(cfg))
                np.random.seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if side == "loop":
                    n_steps = len(sequential_loop(ebos, cfg, events, frames, solv, tmp))
                else:
                    n_steps = len(RecordingEvaluator(cfg, events, frames, solv, save_dir=tmp).run(max_batch=mb).steps)
                torch.cuda.synchronize()
                if rep:
                    times[side].append((time.perf_counter() - t0) / n_steps)
        row = {"size": size, "solver": kind, "max_batch": mb, "n_iter": n_iter, "steps": n_steps, "events_per_window": per}
        for side, v in times.items():
            row[side + "_ms_per_step"] = [1e3 * x for x in v]
            row[side + "_best_ms"], row[side + "_spread_ms"] = 1e3 * min(v), 1e3 * (max(v) - min(v))
        # the conditions: faster than the loop by more than the loop's spread at max_batch 8; not slower beyond it at max_batch 1
        gain = row["loop_best_ms"] - row["evaluator_best_ms"]
        row["gain_ms"] = gain
        row["condition"] = ("faster by more than the loop's spread" if gain > row["loop_spread_ms"] else
                            ("within the loop's spread" if gain >= -row["loop_spread_ms"] else "SLOWER than the loop beyond its spread"))
        rows.append(row)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("per_step")}), flush=True)
    return rows


class HiddenPreparedPath(object):
    """A solver without its ``estimate_batch_prepared``: the evaluator then drives it window by window."""

    def __init__(self, solver):
        object.__setattr__(self, "_solver", solver)

    def __getattr__(self, name):
        if name == "estimate_batch_prepared":
            raise AttributeError(name)
        return getattr(object.__getattribute__(self, "_solver"), name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, "_solver"), name, value)


def cmax_time_aware_solver(shape, n_iter):
    here = os.path.dirname(os.path.abspath(__file__))
    solver = run_eval.load_config(os.path.join(os.path.dirname(here), "configs", "cmax_time_aware_eval.yaml"))["solver"]
    solver["optimizer"]["n_iter"] = n_iter
    size = [max(8, shape[0] // 8), max(8, shape[1] // 8)]
    solver["patch"] = {"size": size, "sliding_window": size}
    return solver


def bench_cmax_time_aware(ebos, size, max_batches, n_iter, repeats, n_frames):
    """The evaluator with the batched prepared path against the same evaluator driving the solver window by window."""
    import torch
    from event_based_bos_amd.evaluation import RecordingEvaluator, synthetic_recording

    shape, roi, per = GEOMETRY[size]
    tmp = tempfile.mkdtemp(prefix="ebos_bench_eval_")
    ev_path, fr_path, tr_path, stamps = synthetic_recording(tmp, shape, n_frames, per)
    cfg = run_eval.synthetic_config(shape, roi, stamps, n_iter)
    cfg["solver"] = cmax_time_aware_solver(shape, n_iter)
    cfg = ebos.utils.propagate_config(cfg)
    events, frames = ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path)
    os.chdir(tmp)
    rows = []
    for mb in max_batches:
        times = {"sequential": [], "prepared": []}
        n_steps = None
        for rep in range(repeats + 1):   # (rep 0 warms both sides up)
            for side in ("sequential", "prepared"):
                solv = run_eval.build_solver(ebos, copy.deepcopy(cfg))
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                driven = HiddenPreparedPath(solv) if side == "sequential" else solv
                n_steps = len(RecordingEvaluator(cfg, events, frames, driven, save_dir=tmp).run(max_batch=mb).steps)
                stop.record()
                stop.synchronize()
                if rep:
                    times[side].append(start.elapsed_time(stop) / n_steps)
        row = {"size": size, "solver": "cmax_time_aware", "max_batch": mb, "n_iter": n_iter, "steps": n_steps, "events_per_window": per,
               "unit": "ms per step (device events around the whole run)"}
        for side, v in times.items():
            row[side] = {"best": round(min(v), 3), "min_max": [round(min(v), 3), round(max(v), 3)], "rounds": [round(x, 3) for x in v]}
        (lo_s, hi_s), (lo_p, hi_p) = row["sequential"]["min_max"], row["prepared"]["min_max"]
        row["verdict"] = "faster" if hi_p < lo_s else ("SLOWER" if lo_p > hi_s else "intervals overlap: no difference counted")
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def ingest_only(ebos, size, repeats):
    import torch
    from event_based_bos_amd.evaluation import window_ingest_raw_batch

    shape, roi, per = GEOMETRY[size]
    rs = np.random.RandomState(0)
    n = per * 8
    store = ebos.RawEventStore({"x": rs.randint(0, shape[1], n).astype(np.int16), "y": rs.randint(0, shape[0], n).astype(np.int16),
                                "t": np.sort(rs.randint(0, 80_000, n)).astype(np.int32), "p": rs.randint(0, 2, n).astype(bool)})
    ranges = [(i * per, (i + 1) * per) for i in range(8)]
    solv = ebos.solver.SolverBase(shape, (roi[1] - roi[0], roi[3] - roi[2]), None,
                                  {"filter": {"parameters": dict(zip(("xmin", "xmax", "ymin", "ymax"), roi))}})
    imager = ebos.EventImageConverter(shape)
    out = {"size": size, "events_per_window": per, "new_ms_per_window": [], "old_ms_per_window": []}
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cols = store.load_raw(0, n)
        window_ingest_raw_batch(cols, ranges, shape, roi, None, 1e6)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for lo, hi in ranges:
            ev, _ = solv.preprocess(store.load_event(lo, hi))
            imager.create_image_from_events_numpy(ev, method="polarity", sigma=0)
            imager.create_eventmask(ev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            out["new_ms_per_window"].append(1e3 * (t1 - t0) / 8)
            out["old_ms_per_window"].append(1e3 * (t2 - t1) / 8)
    # bytes the two launches must move per window: 9 B per event read, the uint32 count image of the CROP box zeroed, added to
    # and read (3 x 8 B per box pixel), pol (16 B) and mask (1 B) written per sensor pixel -- against a device copy of as many bytes
    box = (roi[1] - roi[0]) * (roi[3] - roi[2])
    nbytes = 9 * per + 24 * box + 17 * shape[0] * shape[1]
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    best = float("inf")
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            dst.copy_(src)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / 20)
    out["bytes_per_window"], out["copy_of_as_many_bytes_us"] = nbytes, 1e6 * best
    print(json.dumps({k: (min(v) if isinstance(v, list) else v) for k, v in out.items()}), flush=True)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="260,720")
    ap.add_argument("--solvers", default="pyramid,dependent")
    ap.add_argument("--max-batch", default="1,4,8")
    ap.add_argument("--n-iter", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=11, help="frames of the synthetic recording (steps = frames - 3)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ingest-only", action="store_true")
    args = ap.parse_args(argv)
    import event_based_bos_amd as ebos

    out_path = os.path.abspath(args.out) if args.out else None
    sizes = [int(v) for v in args.shapes.split(",")]
    kinds = args.solvers.split(",")
    only_cmax = kinds == ["cmax_time_aware"]
    result = {"ingest": [] if only_cmax else [ingest_only(ebos, s, args.repeats) for s in sizes], "evaluation": []}
    if not args.ingest_only:
        for s in sizes:
            for kind in kinds:
                if kind == "cmax_time_aware":
                    result["evaluation"] += bench_cmax_time_aware(ebos, s, [int(v) for v in args.max_batch.split(",")], args.n_iter,
                                                                  args.repeats, args.frames)
                    continue
                result["evaluation"] += bench_case(ebos, s, kind, [int(v) for v in args.max_batch.split(",")], args.n_iter,
                                                   args.repeats, args.frames)
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
