#!/usr/bin/env python3
"""Timing of the flow-error metrics (event_based_bos_amd/flow_error.py, csrc/flow_error.hip).

    python tools/bench_flow_error.py [--out profiles/flow_error_bench.json] [--reps 50]
    rocprofv3 --kernel-trace --stats -d <dir> -o fe -- python tools/bench_flow_error.py --kernels-only   # kernel times

(a) the driver's call (bos_event.py:210-219 -> SolverBase.calculate_flow_error): the 720 x 640 ROI of 720 x 1280 float64 numpy
    flows with the event mask of 100 k events, wall clock to the returned dict, against a numpy restatement of the reference's
    function (tests/_flow_error_cases.py) on the same host.
(b) device tensors, B in {1, 8, 64}, float32 and float64 at 720 x 640: time per call from device events around a loop of calls,
    and bytes / time against the 8 TB/s HBM peak (bytes = B * 2 * 2 * H * W * element size + the uint8 mask).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import event_based_bos_amd as ebos  # noqa: E402
from _flow_error_cases import restated_flow_error, solver_events  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
H, W = 720, 640
ROI = {"xmin": 0, "xmax": 720, "ymin": 320, "ymax": 960}


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def driver_call(reps):
    rs = np.random.RandomState(0)
    gt = rs.uniform(-8, 8, (2, 720, 1280))
    pred = gt + rs.normal(0, 2, gt.shape)
    events = solver_events(100_000)
    solver = ebos.solver.SolverBase((720, 1280), (720, 640), solver_config={})
    r = (slice(None), slice(0, 720), slice(320, 960))
    gpu = wall(lambda: solver.calculate_flow_error(pred[r], gt[r], events=events, roi=ROI), reps)
    gpu_nomask = wall(lambda: solver.calculate_flow_error(pred[r], gt[r]), reps)
    mask = solver.orig_imager.create_eventmask(torch.from_numpy(events).cuda())[:, r[1], r[2]].cpu().numpy()
    host = wall(lambda: restated_flow_error(gt[r][None], pred[r][None], mask), max(3, reps // 5))
    return {"gpu_with_mask_ms": gpu[0] * 1e3, "gpu_without_mask_ms": gpu_nomask[0] * 1e3, "host_restatement_ms": host[0] * 1e3,
            "speedup_with_mask": host[0] / gpu[0], "note": "median wall clock; the GPU call includes the upload of the ROI flows "
            "and the event mask built on the device from the events"}


def device_batches(reps, kernels_only=False):
    fe = ebos.flow_error
    rows = []
    for B in (1, 8, 64):
        for dtype in (torch.float32, torch.float64):
            g = torch.randn((B, 2, H, W), dtype=dtype, device="cuda") * 4
            p = g + torch.randn_like(g)
            m = torch.rand((B, 1, H, W), device="cuda") < 0.3
            fe.flow_error_batch(g, p, m)
            torch.cuda.synchronize()
            if kernels_only:
                for _ in range(reps):
                    fe.flow_error_batch(g, p, m)
                torch.cuda.synchronize()
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fe.flow_error_batch(g, p, m)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) / reps * 1e-3
            nbytes = B * 2 * 2 * H * W * g.element_size() + B * H * W
            rows.append({"B": B, "dtype": str(dtype).replace("torch.", ""), "us_per_call": t * 1e6, "bytes": nbytes,
                         "TB_per_s": nbytes / t / 1e12, "share_of_8TBps": nbytes / t / HBM_BYTES_PER_S})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernels-only", action="store_true", help="only the (b) launches, for a rocprofv3 kernel trace")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flow_error needs a GPU"
    if args.kernels_only:
        device_batches(args.reps, kernels_only=True)
        return
    res = {"device": torch.cuda.get_device_name(0), "driver_call": driver_call(args.reps)}
    print(json.dumps(res["driver_call"]), flush=True)
    res["device_batches"] = device_batches(args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
