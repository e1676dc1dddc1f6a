#!/usr/bin/env python3
"""Timing of the time-aware warp on the hot path (csrc/warp_voxel.hip, EventPlan.iwe_voxel / contrast_voxel).

    python tools/bench_warp_voxel.py [--out profiles/warp_voxel_bench.json] [--rounds 5] [--reps 10]

Per shape (2 M events at 1280 x 720, 100 k events at 346 x 260) and ``time_bin`` (1, 5, 15), on one GPU, plan tile (64, 64):

  forward            ``plan.iwe_voxel`` on the tiled route (built halo 32) and on the general route (global atomics), beside
                     ``plan.iwe_dense`` on the same plan (the route without bins: what the bin dimension costs) and the restatement
                     (tests/_warp_voxel_ref.py) as eager torch on the same GPU with the bins kept on the device
  forward + backward ``plan.contrast_voxel(.., "image_variance").backward()`` beside ``plan.contrast_dense`` and eager autograd
  backward alone     ``ebos_iwe_voxel_bwd_f32`` with the segmented wave reduction (``sorted``) and with plain atomics on the same
                     binned plan: whether the reduction still pays when a pixel's events are spread over the bins
  chain              flow -> ``flow_voxel_batch`` (upwind, middle) -> ``contrast_voxel`` -> gradient on the flow, beside eager autograd
                     through tests/_flow_voxel_grad_ref.py and the restatement

Times are device events around a loop of calls, taken in alternating rounds; ``min`` is the best round, [min, max] the spread.  A
difference counts only where the two [min, max] intervals do not overlap (``overlap`` lists the pairs that do).  The rules of
tools/bench_flow_voxel.py.  Values are compared before anything is timed (relative L2 of the IWE, printed per row, not judged here:
tests/test_gpu_warp_voxel.py does that against the CPU)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _flow_voxel_grad_ref as GR  # noqa: E402
import _warp_voxel_ref as R  # noqa: E402
from oracle import ebos_oracle as O  # noqa: E402
import event_based_bos_amd as ebos  # noqa: E402
from event_based_bos_amd import event_plan as EP  # noqa: E402

CASES = [((720, 1280), 2_000_000), ((260, 346), 100_000)]
BINS = (1, 5, 15)


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


def compare(calls, rounds, reps):
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(event_time(fn, reps if not k.startswith("eager") else max(2, reps // 5)))
    row = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    names = list(row)
    row["overlap"] = [[a, b] for i, a in enumerate(names) for b in names[i + 1:]
                      if not (row[a]["max"] < row[b]["min"] or row[b]["max"] < row[a]["min"])]
    return row


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def rows(rounds, reps):
    out = []
    for (H, W), n in CASES:
        ev = torch.from_numpy(O.synth_events(n, H, W, seed=7, tmin=0.0, tmax=1.0)).cuda()
        ev32 = ev.float()
        for T in BINS:
            plan = ebos.EventPlan.build(ev, (H, W), "first", True, tile=(64, 64), emit="full", time_bin=T)
            rs = np.random.RandomState(T)
            vox = torch.from_numpy(rs.uniform(-6.0, 6.0, (T, 2, H, W)).astype(np.float32)).cuda()
            flow = vox[T // 2].contiguous()
            k = torch.from_numpy(R.time_bins(ev[:, 2].cpu().numpy(), T)).cuda()[None]
            base = {"shape": [H, W], "events": n, "time_bin": T, "tile": [64, 64], "unit": "us per call"}

            def eager_iwe(v=vox):
                return R.iwe_voxel(ev32, v, "first", True, bins=k)

            want = eager_iwe()
            row = dict(base, what="forward", rel_l2_tiled_vs_eager=rel(plan.iwe_voxel(vox), want),
                       rel_l2_general_vs_eager=rel(plan.iwe_voxel(vox, halo=None), want))
            row.update(compare({"voxel_tiled": lambda: plan.iwe_voxel(vox), "voxel_general": lambda: plan.iwe_voxel(vox, halo=None),
                                "dense_same_plan": lambda: plan.iwe_dense(flow), "dense_general": lambda: plan.iwe_dense(flow, halo=None),
                                "eager_torch": eager_iwe}, rounds, reps))
            print(json.dumps(row), flush=True)
            out.append(row)

            vg, fg = vox.clone().requires_grad_(True), flow.clone().requires_grad_(True)

            def fb_voxel(halo):
                vg.grad = None
                plan.contrast_voxel(vg, "image_variance", halo=halo).backward()

            def fb_dense(halo):
                fg.grad = None
                plan.contrast_dense(fg, "image_variance", halo=halo).backward()

            def fb_eager():
                vg.grad = None
                R.image_variance(R.iwe_voxel(ev32, vg, "first", True, bins=k)).backward()

            row = dict(base, what="forward + backward (variance)")
            row.update(compare({"voxel_tiled": lambda: fb_voxel(32), "voxel_general": lambda: fb_voxel(None), "dense_same_plan": lambda: fb_dense(32),
                                "dense_general": lambda: fb_dense(None), "eager_torch": fb_eager}, rounds, reps))
            print(json.dumps(row), flush=True)
            out.append(row)

            g = plan.iwe_voxel(vox).contiguous()
            row = dict(base, what="backward alone: segmented reduction (sorted) against plain atomics, binned plan")
            row.update(compare({"sorted": lambda: EP._launch_voxel_bwd(plan, vox, None, (0, 0), g, None, 0, False, sorted_=True),
                                "plain_atomics": lambda: EP._launch_voxel_bwd(plan, vox, None, (0, 0), g, None, 0, False, sorted_=False)},
                               rounds, reps))
            print(json.dumps(row), flush=True)
            out.append(row)

            if T > 1:
                f0 = torch.from_numpy(rs.uniform(0.5, 3.0, (2, H, W)).astype(np.float32)).cuda().requires_grad_(True)

                def chain():
                    f0.grad = None
                    plan.contrast_voxel(ebos.flow_voxel_batch(f0[None], T, "upwind", "middle")[0], "image_variance").backward()

                def chain_eager():
                    f0.grad = None
                    R.image_variance(R.iwe_voxel(ev32, GR.voxel_torch(f0[None], T, "upwind", "middle")[0], "first", True, bins=k)).backward()

                chain()
                got = f0.grad.clone()
                chain_eager()
                row = dict(base, what="chain: flow -> voxel (upwind, middle) -> contrast -> gradient", rel_l2_gradient_vs_eager=rel(got, f0.grad))
                row.update(compare({"kernels": chain, "eager_torch": chain_eager}, rounds, reps))
                print(json.dumps(row), flush=True)
                out.append(row)
            plan.clear_cache()
            del plan
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_voxel_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_warp_voxel needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
           "method": "device events around a loop of calls; alternating rounds; best round (min) and [min, max] over the rounds",
           "rows": rows(args.rounds, args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
