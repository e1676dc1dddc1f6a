#!/usr/bin/env python3
"""Timing of the time-aware objective at K reference times (csrc/warp_voxel_multiref.hip, the K-reference loop of csrc/cmax_voxel.hip,
solver/time_aware_loop.py).

    python tools/bench_voxel_multiref.py [--out profiles/voxel_multiref_bench.json] [--rounds 5] [--reps 3] [--iters 50]

Per shape (2 M events at 1280 x 720, 100 k events at 346 x 260) and ``time_bin`` (5, 15), on one GPU, K = 3 (first, middle, last), plan
tile (64, 64), patch (24, 32), scheme upwind, t0 in the middle, a patch grid drawn in [0.5, 3]:

  forward + backward  microseconds per evaluation of mean_k var(IWE_k(voxel)) and its gradient with respect to the voxel
                        multiref          ``EventPlan.variance_voxel_multi_value_and_grad``: one K-image forward, one K-reference owner backward
                        three_plans       what the code could do before: three binned plans built with the three directions, each through
                                          ``variance_voxel_value_and_grad`` (upstream 1 / 3), the three d_voxel added
                        autograd          ``contrast_voxel_multi(...).backward()`` on a leaf voxel
  loop                microseconds per Adam iteration of one pyramid scale
                        native            ``TimeAwareMultiReferencePatchLoop.run(iters)`` on a loop built once (state reset per call)
                        solver_native / solver_autograd   ``ContrastMaximization._optimise_patch_grid`` with ``time_aware.directions`` and
                                          ``native`` true / false (whatever it allocates, its loop and the read-back of the losses)

Times are device events around a loop of calls, taken in alternating rounds; ``min`` is the best round, [min, max] the spread.  A
difference counts only where the two [min, max] intervals do not overlap (``overlap`` lists the pairs that do).  The rules of
tools/bench_voxel_loop.py.  The values of the variants are compared before anything is timed (printed per row, not judged here:
tests/test_gpu_voxel_multiref.py does that against the CPU)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ebos_oracle as O  # noqa: E402
import event_based_bos_amd as ebos  # noqa: E402
from event_based_bos_amd import ops  # noqa: E402
from bench_voxel_loop import BINS, CASES, PATCH, TILE, compare  # noqa: E402
from event_based_bos_amd.flow_voxel import flow_voxel_batch  # noqa: E402
from event_based_bos_amd.solver.contrast_maximization import patch_grid_shape  # noqa: E402
from event_based_bos_amd.solver.time_aware_loop import TimeAwareMultiReferencePatchLoop  # noqa: E402

DIRECTIONS = ["first", "middle", "last"]


def solver_of(shape, T, native, iters):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0, "tile": list(TILE),
           "patch": {"size": list(PATCH), "sliding_window": list(PATCH)},
           "optimizer": {"method": "Adam", "n_iter": iters, "parameters": {"lr": 0.05}},
           "time_aware": {"time_bin": T, "scheme": "upwind", "t0_location": "middle", "native": native, "directions": DIRECTIONS}}
    return ebos.solver.collections["contrast_maximization"](shape, shape, solver_config=cfg)


def rows(rounds, reps, iters):
    out = []
    K = len(DIRECTIONS)
    for (H, W), n in CASES:
        ev = torch.from_numpy(O.synth_events(n, H, W, seed=7, tmin=0.0, tmax=1.0)).cuda()
        gh, gw = patch_grid_shape((H, W), PATCH, PATCH)
        theta0 = torch.from_numpy(np.random.RandomState(3).uniform(0.5, 3.0, (2, gh, gw)).astype(np.float32)).cuda()
        for T in BINS:
            plans = {d: ebos.EventPlan.build(ev, (H, W), d, True, tile=TILE, emit="full", time_bin=T) for d in DIRECTIONS}
            plan = plans["first"]
            base = {"shape": [H, W], "events": n, "time_bin": T, "K": K, "directions": DIRECTIONS, "tile": list(TILE), "patch": list(PATCH)}
            dense = ops.upsample_patch_flow(theta0, PATCH, PATCH, (H, W))
            voxel = flow_voxel_batch(dense[None], T, "upwind", "middle", None)[0].contiguous()
            d_multi = torch.empty_like(voxel)
            d_parts = [torch.empty_like(voxel) for _ in DIRECTIONS]
            leaf = voxel.clone().requires_grad_(True)
            results = {}

            def multiref():
                results["multiref"] = plan.variance_voxel_multi_value_and_grad(voxel, DIRECTIONS, out=d_multi)

            def three_plans():
                values = [plans[d].variance_voxel_value_and_grad(voxel, upstream=1.0 / K, out=d_parts[k])[0] for k, d in enumerate(DIRECTIONS)]
                results["three_plans"] = (sum(values) / K, d_parts[0] + d_parts[1] + d_parts[2])

            def autograd():
                leaf.grad = None
                value = plan.contrast_voxel_multi(leaf, DIRECTIONS)
                value.backward()
                results["autograd"] = (value.detach(), leaf.grad)

            calls = {"multiref": multiref, "three_plans": three_plans, "autograd": autograd}
            for fn in calls.values():
                fn()
            ref_v, ref_d = float(results["three_plans"][0]), results["three_plans"][1].double()
            row = dict(base, what="forward + backward: mean_k var(IWE_k) and d_voxel", unit="us per evaluation",
                       value_rel_to_three_plans={k: abs(float(v[0]) - ref_v) / abs(ref_v) for k, v in results.items()},
                       d_voxel_rel_l2_to_three_plans={k: float((v[1].double() - ref_d).norm() / ref_d.norm()) for k, v in results.items()})
            row.update(compare(calls, rounds, max(reps, 10)))
            print(json.dumps(row), flush=True)
            out.append(row)

            # the Adam loop of one pyramid scale
            ta = {"time_bin": T, "scheme": "upwind", "t0_location": "middle", "clamp": None, "directions": DIRECTIONS}
            loop = TimeAwareMultiReferencePatchLoop(plan, PATCH, PATCH, theta0, ta, 1.0, lr=0.05, capacity=iters)

            def run_loop():
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

            run_loop()
            losses = {"native": loop.losses[:iters].cpu().numpy().astype(np.float64)}
            for k, slv in solvers.items():
                run_solver(slv)
                losses[k] = np.array(slv.history)
            ref = losses["solver_autograd"]
            row = dict(base, what="loop", unit="us per iteration", iterations_per_call=iters, modes={k: s.loop_mode for k, s in solvers.items()},
                       first_loss_rel_to_autograd={k: float(abs(v[0] - ref[0]) / abs(ref[0])) for k, v in losses.items()},
                       last_loss_rel_to_autograd={k: float(abs(v[-1] - ref[-1]) / abs(ref[-1])) for k, v in losses.items()})
            calls = {"native": run_loop}
            calls.update({k: (lambda s=s: run_solver(s)) for k, s in solvers.items()})
            row.update(compare(calls, rounds, reps, per=iters))
            print(json.dumps(row), flush=True)
            out.append(row)
            del loop, solvers
            for p in plans.values():
                p.clear_cache()
            del plans, plan
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_multiref_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel_multiref needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "iters": args.iters,
           "method": "device events around a loop of calls; alternating rounds; best round (min) and [min, max] over the rounds",
           "rows": rows(args.rounds, args.reps, args.iters)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
