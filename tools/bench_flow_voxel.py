#!/usr/bin/env python3
"""Timing of the flow voxels (event_based_bos_amd/flow_voxel.py, csrc/flow_voxel.hip).

    python tools/bench_flow_voxel.py [--out profiles/flow_voxel_bench.json] [--rounds 5] [--reps 20]
    python tools/bench_flow_voxel.py --backward [--out profiles/flow_voxel_backward_bench.json]

Per shape (260 x 346, 720 x 1280), ``time_bin`` (5, 15), batch (1, 8), scheme (upwind, burgers) and dtype (float32, float64), with t0 in
the middle: ``flow_voxel_batch`` on device tensors against the restatement of the reference's constructor (tests/_flow_voxel_ref.py:
a Python loop of ``time_bin - 1`` stencil steps, each some twenty full-image temporaries) run as eager torch on the same GPU, in the
same process, per flow.  The forced per-step route is timed beside the fused one.

Times are device events around a loop of calls, taken in alternating rounds (kernel, per-step, eager, kernel, ...); the median over
the rounds and their spread (min, max) are kept.  A difference counts as a gain only where the two [min, max] intervals do not
overlap; ``intervals_overlap`` says so per row.  ``copy_share`` is the time a device-to-device copy at the measured rate needs for
the bytes the chain must move (read 2 H W, write 2 T H W elements per flow), divided by the kernel's time: 1.0 is a kernel as fast as
a copy of its output.

``--backward`` times forward plus backward per voxel instead (csrc/flow_voxel_grad.hip): 260 x 346 and 720 x 1280, ``time_bin`` 5 and
17, batch 1 and 8, the four schemes, float32 and float64, against eager torch on the same GPU running the restatement of the
reference's expressions under autograd (tests/_flow_voxel_grad_ref.py), in the same process and in alternating rounds.  ``min`` is the
best round, [min, max] the spread.  ``relative_difference`` is max|kernel - eager| / max|eager| of the two gradients, reported and not
judged here (tests/test_gpu_flow_voxel_grad.py does that against the CPU).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _flow_voxel_ref as R  # noqa: E402
import _flow_voxel_grad_ref as GR  # noqa: E402
from event_based_bos_amd import _hip  # noqa: E402
from event_based_bos_amd import flow_voxel as FV  # noqa: E402

SHAPES = [(260, 346), (720, 1280)]
BINS = (5, 15)
BATCHES = (1, 8)


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
    return e0.elapsed_time(e1) / reps * 1e3   # microseconds


def stats(values):
    v = np.array(values)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def compare(calls, rounds, reps, per=1):
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(event_time(fn, reps) / per)
    row = {k: stats(v) for k, v in times.items()}
    a, b = row["kernel"], row["eager_torch"]
    row["intervals_overlap"] = not (a["max"] < b["min"] or b["max"] < a["min"])
    return row


def copy_rate(rounds, reps):
    """Bytes per microsecond a device-to-device copy moves (read + write), on 256 MiB: far beyond the Infinity Cache."""
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    us = [event_time(lambda: dst.copy_(src), reps) for _ in range(rounds)]
    return 2.0 * src.numel() / float(np.median(us))


def forced(route, *args):
    FV._FORCE_ROUTE = route
    try:
        return FV.flow_voxel_batch(*args)
    finally:
        FV._FORCE_ROUTE = None


def rows(rounds, reps, rate):
    out = []
    rs = np.random.RandomState(0)
    for H, W in SHAPES:
        for dtype in (torch.float32, torch.float64):
            for B in BATCHES:
                flows = torch.from_numpy(rs.uniform(-3.0, 3.0, (B, 2, H, W))).cuda().to(dtype)
                for T in BINS:
                    for scheme in ("upwind", "burgers"):
                        # the yardstick is the restatement on the CPU; eager torch on the GPU is only timed, and whether its
                        # elementwise kernels round every operation on its own is reported, not presumed
                        got, eager = FV.flow_voxel_batch(flows, T, scheme, "middle"), R.construct(flows, T, scheme, "middle")
                        want = R.construct(flows.cpu(), T, scheme, "middle")
                        assert torch.equal(got.cpu(), want), "the kernel and the CPU restatement disagree"
                        assert torch.allclose(eager.cpu(), want, rtol=1e-4, atol=1e-4), "the eager restatement on the GPU is off"
                        eager_bit_equal = bool(torch.equal(eager.cpu(), want))
                        buf = torch.empty_like(got)
                        row = {"shape": [H, W], "dtype": str(dtype).split(".")[-1], "B": B, "time_bin": T, "scheme": scheme,
                               "unit": "us per flow", "eager_torch_bit_equal": eager_bit_equal}
                        row.update(compare({"kernel": lambda: FV.flow_voxel_batch(flows, T, scheme, "middle", None, buf),
                                            "per_step_route": lambda: forced(_hip.FLOW_ROUTE_STEPS, flows, T, scheme, "middle", None, buf),
                                            "eager_torch": lambda: R.construct(flows, T, scheme, "middle")}, rounds, reps, per=B))
                        must_move = (2 + 2 * T) * H * W * flows.element_size()
                        row["bytes_per_flow"] = must_move
                        row["copy_share"] = (must_move / rate) / row["kernel"]["median"]
                        print(json.dumps(row), flush=True)
                        out.append(row)
                        del got, want, eager, buf
    return out


def backward_rows(rounds, reps):
    out = []
    rs = np.random.RandomState(1)
    for H, W in SHAPES:
        for dtype in (torch.float32, torch.float64):
            for B in BATCHES:
                flows = torch.from_numpy(rs.uniform(-3.0, 3.0, (B, 2, H, W))).cuda().to(dtype).requires_grad_()
                for T in (5, 17):
                    up = torch.from_numpy(rs.standard_normal((B, T, 2, H, W))).cuda().to(dtype)
                    for scheme in ("upwind", "burgers", "same", "bilinear"):
                        def kernel(route=None):
                            flows.grad = None
                            FV._FORCE_ROUTE = route
                            try:
                                FV.flow_voxel_batch(flows, T, scheme, "middle").backward(up)
                            finally:
                                FV._FORCE_ROUTE = None
                            return flows.grad

                        def eager():
                            flows.grad = None
                            GR.voxel_torch(flows, T, scheme, "middle").backward(up)
                            return flows.grad

                        got, want = kernel(), eager()
                        scale = float(want.abs().max())
                        worst = float((got - want).abs().max()) / scale
                        row = {"shape": [H, W], "dtype": str(dtype).split(".")[-1], "B": B, "time_bin": T, "scheme": scheme,
                               "unit": "us per voxel, forward + backward", "relative_difference": worst}
                        calls = {"kernel": kernel, "eager_torch": eager}
                        if scheme in ("upwind", "burgers"):
                            calls["per_step_route"] = lambda: kernel(_hip.FLOW_ROUTE_STEPS)
                        row.update(compare(calls, rounds, reps, per=B))
                        row["speedup_of_best"] = row["eager_torch"]["min"] / row["kernel"]["min"]
                        print(json.dumps(row), flush=True)
                        out.append(row)
                        del got, want
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backward", action="store_true", help="time forward + backward against eager autograd instead of the forward")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "flow_voxel_backward_bench.json" if args.backward else "flow_voxel_bench.json")
    assert torch.cuda.is_available(), "bench_flow_voxel needs a GPU"
    if args.backward:
        res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
               "method": "device events around a loop of forward + backward calls; alternating rounds; median and [min, max] over the rounds",
               "rows": backward_rows(args.rounds, args.reps)}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
        return
    rate = copy_rate(args.rounds, args.reps)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "copy_bytes_per_us": rate,
           "method": "device events around a loop of calls; alternating rounds; median and [min, max] over the rounds"}
    print(json.dumps({"copy_GB_per_s": rate / 1e3}), flush=True)
    res["rows"] = rows(args.rounds, args.reps, rate)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
