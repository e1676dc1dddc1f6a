#!/usr/bin/env python3
"""Timing of the native time-aware loop (solver/time_aware_loop.py, csrc/cmax_voxel.hip) and of the pixel-owner backward into the flow
voxel (``ebos_iwe_voxel_owner_bwd_f32``, csrc/warp_voxel.hip).

    python tools/bench_voxel_loop.py [--out profiles/voxel_loop_bench.json] [--rounds 5] [--reps 3] [--iters 50]

Per shape (2 M events at 1280 x 720, 100 k events at 346 x 260) and ``time_bin`` (5, 15), on one GPU, plan tile (64, 64), patch
(24, 32), scheme upwind, t0 in the middle, a patch grid drawn in [0.5, 3]:

  loop            microseconds per Adam iteration of
                    native_owner / native_atomic   ``TimeAwarePatchLoop.run(iters)`` on a loop built once (state reset per call), with the
                                                   owner backward and with memset + ``ebos_iwe_voxel_bwd_f32``
                    solver_native / solver_autograd  one pyramid scale of ``ContrastMaximization`` (``_optimise_patch_grid``: whatever it
                                                   allocates, its loop and the read-back of the losses) with ``time_aware.native`` true and
                                                   false -- the second is the loop the solver ran before, in the same process
  backward alone  ``ebos_iwe_voxel_owner_bwd_f32`` into a caller-owned buffer against a zero-fill of that buffer +
                  ``ebos_iwe_voxel_bwd_f32`` (sorted: the segmented wave reduction)

With ``--batch B`` the tool measures the batch loop instead (``TimeAwarePatchLoopBatch``: ``ebos_cmax_voxel_solve_batch_f32``): per case
one row "per window, one batch solve of B windows" against "the loop of B single native solves" (B windows of the case's size drawn
with B seeds, each with its own start grid; the backward ``default_owner_bwd`` picks), both per window and per iteration, through the
same ``compare``; the raw output goes to profiles/voxel_loop_batch_bench.json.

Times are device events around a loop of calls, taken in alternating rounds; ``min`` is the best round, [min, max] the spread.  A
difference counts only where the two [min, max] intervals do not overlap (``overlap`` lists the pairs that do).  The rules of
tools/bench_warp_voxel.py.  The losses of the variants are compared before anything is timed (printed per row, not judged here:
tests/test_gpu_voxel_loop.py does that against the CPU)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ebos_oracle as O  # noqa: E402
import event_based_bos_amd as ebos  # noqa: E402
from event_based_bos_amd import _hip  # noqa: E402
from event_based_bos_amd._hip import check, ptr, stream_ptr  # noqa: E402
from event_based_bos_amd.solver.contrast_maximization import patch_grid_shape  # noqa: E402
from event_based_bos_amd.solver.time_aware_loop import TimeAwarePatchLoop, TimeAwarePatchLoopBatch  # noqa: E402

CASES = [((720, 1280), 2_000_000), ((260, 346), 100_000)]
BINS = (5, 15)
PATCH = (24, 32)
TILE = (64, 64)


def event_time(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # microseconds


def compare(calls, rounds, reps, per=1):
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(event_time(fn, reps) / per)
    row = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    names = list(row)
    row["overlap"] = [[a, b] for i, a in enumerate(names) for b in names[i + 1:]
                      if not (row[a]["max"] < row[b]["min"] or row[b]["max"] < row[a]["min"])]
    return row


def solver_of(shape, T, native, iters):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0, "tile": list(TILE),
           "patch": {"size": list(PATCH), "sliding_window": list(PATCH)},
           "optimizer": {"method": "Adam", "n_iter": iters, "parameters": {"lr": 0.05}},
           "time_aware": {"time_bin": T, "scheme": "upwind", "t0_location": "middle", "native": native}}
    return ebos.solver.collections["contrast_maximization"](shape, shape, solver_config=cfg)


def rows(rounds, reps, iters):
    out = []
    lib = _hip.require_gpu()
    for (H, W), n in CASES:
        ev = torch.from_numpy(O.synth_events(n, H, W, seed=7, tmin=0.0, tmax=1.0)).cuda()
        gh, gw = patch_grid_shape((H, W), PATCH, PATCH)
        theta0 = torch.from_numpy(np.random.RandomState(3).uniform(0.5, 3.0, (2, gh, gw)).astype(np.float32)).cuda()
        for T in BINS:
            plan = ebos.EventPlan.build(ev, (H, W), "first", True, tile=TILE, emit="full", time_bin=T)
            base = {"shape": [H, W], "events": n, "time_bin": T, "tile": list(TILE), "patch": list(PATCH), "iterations_per_call": iters}
            ta = {"time_bin": T, "scheme": "upwind", "t0_location": "middle", "clamp": None}
            loops = {k: TimeAwarePatchLoop(plan, PATCH, PATCH, theta0, ta, 1.0, lr=0.05, capacity=iters, owner_bwd=o)
                     for k, o in (("native_owner", True), ("native_atomic", False))}

            def run_loop(loop):
                loop.theta.copy_(theta0)
                loop.exp_avg.zero_()
                loop.exp_avg_sq.zero_()
                loop.t = 0
                loop.run(iters)

            solvers = {"solver_native": solver_of((H, W), T, True, iters), "solver_autograd": solver_of((H, W), T, False, iters)}

            def run_solver(slv):
                slv.history, slv.loop_modes = [], []
                with torch.autograd.set_multithreading_enabled(False):
                    slv._optimise_patch_grid(plan, theta0.clone(), PATCH, PATCH, iters, None)

            losses = {}
            for k, loop in loops.items():
                run_loop(loop)
                losses[k] = loop.losses[:iters].cpu().numpy().astype(np.float64)
            for k, slv in solvers.items():
                run_solver(slv)
                losses[k] = np.array(slv.history)
            ref = losses["solver_autograd"]
            row = dict(base, what="loop", unit="us per iteration",
                       modes={k: s.loop_mode for k, s in solvers.items()},
                       last_loss_rel_to_autograd={k: float(abs(v[-1] - ref[-1]) / abs(ref[-1])) for k, v in losses.items()},
                       first_loss_rel_to_autograd={k: float(abs(v[0] - ref[0]) / abs(ref[0])) for k, v in losses.items()})
            calls = {k: (lambda lp=lp: run_loop(lp)) for k, lp in loops.items()}
            calls.update({k: (lambda s=s: run_solver(s)) for k, s in solvers.items()})
            row.update(compare(calls, rounds, reps, per=iters))
            print(json.dumps(row), flush=True)
            out.append(row)

            # the backward alone, on the loop's own state (voxel, IWE and affine map of its last iteration)
            lp = loops["native_owner"]
            d = torch.empty_like(lp.d_voxel)

            def owner():
                check(lib.ebos_iwe_voxel_owner_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), None, ptr(plan.bins), ptr(plan.key_offsets), plan.n,
                                                       ptr(lp.voxel), T, H, W, TILE[0], TILE[1], 0, 0, ptr(lp.iwe), ptr(lp.affine), 0, ptr(d),
                                                       stream_ptr()), "ebos_iwe_voxel_owner_bwd")

            def atomic():
                d.zero_()
                check(lib.ebos_iwe_voxel_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), None, ptr(plan.bins), plan.n, ptr(lp.voxel), T, H, W, W,
                                                 0, 0, ptr(lp.iwe), ptr(lp.affine), 0, 1, ptr(d), None, stream_ptr()), "ebos_iwe_voxel_bwd")

            owner()
            a = d.clone()
            atomic()
            row = dict(base, what="backward alone: owner kernel against zero-fill + sorted atomic kernel", unit="us per call",
                       rel_l2_owner_vs_atomic=float((a.double() - d.double()).norm() / d.double().norm()))
            row.update(compare({"owner": owner, "zero_fill_plus_atomic_sorted": atomic}, rounds, max(reps, 20)))
            print(json.dumps(row), flush=True)
            out.append(row)
            del loops, solvers, lp
            plan.clear_cache()
            del plan
    return out


def batch_rows(B, rounds, reps, iters):
    """Per case: one batch solve of B windows against the loop of B single native solves, microseconds per window and iteration."""
    out = []
    for (H, W), n in CASES:
        gh, gw = patch_grid_shape((H, W), PATCH, PATCH)
        evs = [torch.from_numpy(O.synth_events(n, H, W, seed=7 + b, tmin=0.0, tmax=1.0)).cuda() for b in range(B)]
        theta0 = torch.from_numpy(np.random.RandomState(3).uniform(0.5, 3.0, (B, 2, gh, gw)).astype(np.float32)).cuda()
        for T in BINS:
            plans = [ebos.EventPlan.build(ev, (H, W), "first", True, tile=TILE, emit="full", time_bin=T) for ev in evs]
            ta = {"time_bin": T, "scheme": "upwind", "t0_location": "middle", "clamp": None}
            batch = TimeAwarePatchLoopBatch(plans, PATCH, PATCH, theta0, ta, 1.0, lr=0.05, capacity=iters)
            singles = [TimeAwarePatchLoop(plan, PATCH, PATCH, theta0[b], ta, 1.0, lr=0.05, capacity=iters, owner_bwd=batch.owner_bwd)
                       for b, plan in enumerate(plans)]

            def reset(loop, start):
                loop.theta.copy_(start)
                loop.exp_avg.zero_()
                loop.exp_avg_sq.zero_()
                loop.t = 0

            def run_batch():
                reset(batch, theta0)
                batch.run(iters)

            def run_singles():
                for b, loop in enumerate(singles):
                    reset(loop, theta0[b])
                    loop.run(iters)

            run_batch()
            run_singles()
            got = batch.losses[:, :iters].cpu().numpy().astype(np.float64)
            want = np.stack([loop.losses[:iters].cpu().numpy().astype(np.float64) for loop in singles])
            row = dict(shape=[H, W], events_per_window=n, windows=B, time_bin=T, tile=list(TILE), patch=list(PATCH), iterations_per_call=iters,
                       owner_bwd=bool(batch.owner_bwd), what="per window, one batch solve of B windows against the loop of B single native solves",
                       unit="us per window and iteration",
                       first_loss_rel_to_single=float(np.max(np.abs(got[:, 0] - want[:, 0]) / np.abs(want[:, 0]))),
                       last_loss_rel_to_single=float(np.max(np.abs(got[:, -1] - want[:, -1]) / np.abs(want[:, -1]))))
            row.update(compare({"batch_per_window": run_batch, "single_loop_per_window": run_singles}, rounds, reps, per=iters * B))
            print(json.dumps(row), flush=True)
            out.append(row)
            del batch, singles, plans
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/voxel_loop_bench.json, with --batch profiles/voxel_loop_batch_bench.json")
    ap.add_argument("--batch", type=int, nargs="+", default=None, metavar="B",
                    help="measure the batch loop of B windows (several values: one set of rows each) instead of the single loop's rows")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel_loop needs a GPU"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "voxel_loop_batch_bench.json" if args.batch else "voxel_loop_bench.json")
    if args.batch:
        measured = [r for B in args.batch for r in batch_rows(B, args.rounds, args.reps, args.iters)]
    else:
        measured = rows(args.rounds, args.reps, args.iters)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "iters": args.iters,
           "method": "device events around a loop of calls; alternating rounds; best round (min) and [min, max] over the rounds",
           "rows": measured}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
