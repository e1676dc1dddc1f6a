#!/usr/bin/env python3
"""Timing of the frame-based flow (event_based_bos_amd/frame_flow.py, csrc/farneback.hip) with the YAML's params_opencv_flow.

    python tools/bench_frame_flow.py [--out profiles/frame_flow_bench.json] [--restatement]
    rocprofv3 --kernel-trace --stats -d <dir> -o ff -- python tools/bench_frame_flow.py --quick     # per-kernel times
    python tools/bench_frame_flow.py --merge-stats <dir>/.../ff_kernel_stats.csv [--out ...]          # -> the JSON

(a) uint8 device frames at 720 x 640 (the YAML's ROI crop), 720 x 1280 and 260 x 346, B in {1, 8}: time per pair from device
    events around a loop of calls after warm-up, at least 1 s of work; launches per call and the bytes each level's kernels move,
    computed from the shapes (a lower bound: every buffer read and written once);
(b) the two-step chain (FrameFlowEstimator.opencv_farneback_two_step) at 720 x 1280 on device frames;
(c) with --restatement: the numpy restatement (tests/_farneback_ref.py) on one 720 x 640 pair -- the restatement's time, not
    OpenCV's;
(d) with --quick (under rocprofv3): 720 x 640 at B = 8 only, for the kernel trace; --merge-stats adds the kernel times per pair.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

YAML = {"pyr_scale": 0.5, "levels": 4, "winsize": 10, "iterations": 3, "poly_n": 5, "poly_sigma": 1.2, "flags": 0,
        "pad_x0": 0, "pad_x1": 0, "pad_y0": 0, "pad_y1": 0}
GEOMETRIES = ((720, 640), (720, 1280), (260, 346))
BATCHES = (1, 8)
QUICK = ((720, 640), 8, 20)


def frames(B, H, W, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H // 4 + 2, W // 4 + 2)).astype(np.float32)
    big = np.kron(base, np.ones((4, 4), np.float32))
    out = [big[i % 3:i % 3 + H, 2 * (i % 3):2 * (i % 3) + W] for i in range(B + 1)]
    return torch.from_numpy(np.stack(out).astype(np.uint8)).cuda()


def plan(H, W, p):
    from _farneback_ref import level_plan
    return level_plan(H, W, p["pyr_scale"], p["levels"])


def traffic(B, H, W, p, shared=False):
    """(launches, bytes) of one call: per level, the frame pixels the level image reads (once), the images, R, flow and M planes
    each written once and read once per consumer."""
    launches, total, per_level = 0, 0, []
    nimg = B + (1 if shared else B)
    for lv, s, h, w, sigma, ks in plan(H, W, p):
        hw = h * w
        b = nimg * H * W                                   # the frame is read at least once per level
        b += nimg * hw * 4 * 2                             # level image: write + read by the expansion
        b += nimg * hw * 5 * 4 * 2                         # R: write + read
        b += B * hw * (2 * 4 + 5 * 4)                      # init: flow + M
        b += p["iterations"] * B * hw * (5 * 4 + 2 * 4 + 5 * 4)   # per iteration: M in, flow out, next M out
        launches += 3 + p["iterations"]
        total += b
        per_level.append({"level": lv, "h": h, "w": w, "blur_taps": ks, "bytes": b})
    return launches, total, per_level


def device_time(fn, min_seconds=1.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps, ms = 1, 0.0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1000 * min_seconds:
            return ms / reps, reps
        reps *= 2 if ms < 100 else max(2, int(1000 * min_seconds / ms) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--merge-stats")
    args = ap.parse_args()
    from event_based_bos_amd.frame_flow import FrameFlowEstimator, farneback_batch

    if args.merge_stats:
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        (H, W), B, calls = QUICK
        rows = list(csv.DictReader(open(args.merge_stats)))
        kern = {}
        for r in rows:
            name = r["Name"].split("(")[0].split("<")[0].replace("ebos::(anonymous namespace)::", "")
            kern[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                          "ms_per_pair": float(r["TotalDurationNs"]) / 1e6 / ((calls + 3) * B)}
        res["kernels_720x640_B8"] = kern
        print(json.dumps(kern, indent=1))
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return
    if args.quick:
        (H, W), B, calls = QUICK
        f = frames(B, H, W)
        for _ in range(calls + 3):
            farneback_batch(f[:1], f[1:], YAML)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "params": YAML, "pairs": []}
    for H, W in GEOMETRIES:
        for B in BATCHES:
            f = frames(B, H, W)
            ms, reps = device_time(lambda: farneback_batch(f[:B], f[1:], YAML))
            launches, nbytes, levels = traffic(B, H, W, YAML)
            r = {"H": H, "W": W, "B": B, "ms_per_call": ms, "ms_per_pair": ms / B, "calls_timed": reps,
                 "launches_per_call": launches, "bytes_per_call": nbytes, "GB_per_s": nbytes / (ms * 1e-3) / 1e9,
                 "levels": levels}
            res["pairs"].append(r)
            print(f"{H:4d} x {W:4d} B={B}: {ms / B:.3f} ms/pair ({ms:.3f} ms/call, {launches} launches, "
                  f"{nbytes / 1e6:.0f} MB, {r['GB_per_s']:.0f} GB/s lower bound)", flush=True)
    H, W = 720, 1280
    f = frames(2, H, W).contiguous()
    est = FrameFlowEstimator()
    ms, reps = device_time(lambda: est.opencv_farneback_two_step(f[0], f[1], f[2], YAML))
    res["two_step_720x1280_ms"] = ms
    print(f"two-step chain 720 x 1280: {ms:.3f} ms per call", flush=True)
    if args.restatement:
        import _farneback_ref as R
        a = frames(1, 720, 640).cpu().numpy()
        t = time.perf_counter()
        R.calc_optical_flow_farneback(a[0], a[1], None, *(YAML[k] for k in ("pyr_scale", "levels", "winsize", "iterations",
                                                                             "poly_n", "poly_sigma")))
        res["numpy_restatement_720x640_ms"] = (time.perf_counter() - t) * 1e3
        print(f"numpy restatement (not OpenCV) 720 x 640: {res['numpy_restatement_720x640_ms']:.0f} ms per pair")
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
