#!/usr/bin/env python3
"""Timing of the Poisson integration (event_based_bos_amd/poisson.py, csrc/poisson.hip).

    python tools/bench_poisson.py [--out profiles/poisson_bench.json] [--mfma-json ubench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o po -- python tools/bench_poisson.py --quick        # kernel times
    python tools/bench_poisson.py --merge-stats <dir>/.../po_kernel_stats.csv [--out ...]            # -> the JSON

(a) device tensors, geometries 260 x 346, 640 x 720 and 720 x 1280, B in {1, 8, 64}, float32 and float64 flows: time per call
    from device events around a loop of calls (float64 output: the visualizer's zeros boundary of the flow's dtype would make the
    float32 case's output float32; the arithmetic is float64 either way);
(b) a host restatement with scipy's DSTs in float64 (the reference's algorithm), one flow, on the same node;
(c) with --quick (under rocprofv3): only 720 x 1280 float64 at B = 8, for the kernel trace; --merge-stats then adds the kernel time
    per flow, the achieved TF/s (FLOP = 4 h w (h + w) per flow) and its share of the measured fp64 MFMA rate
    (tools/ubench_mfma_f64.hip, --mfma-json) to the JSON.
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

GEOMETRIES = ((260, 346), (640, 720), (720, 1280))
BATCHES = (1, 8, 64)
QUICK = ((720, 1280), 8, "float64", 20)   # geometry, B, dtype, calls


def flop_per_flow(H, W):
    h, w = H - 2, W - 2
    return 4.0 * h * w * (h + w)


def synth(B, H, W, dtype, seed=0):
    from _poisson_cases import synth_flow
    one = synth_flow(H, W, seed)
    rs = np.random.RandomState(seed + 1)
    return np.stack([one + rs.normal(0, 0.01, one.shape) for _ in range(B)]).astype(dtype)


def device_time(flow, reps):
    from event_based_bos_amd.poisson import poisson_reconstruct_batch
    for _ in range(2):
        poisson_reconstruct_batch(flow, dtype=torch.float64)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        poisson_reconstruct_batch(flow, dtype=torch.float64)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def host_restatement(flow):
    """The reference's algorithm with scipy's orthonormal DSTs, float64, one flow."""
    import scipy.fft as sf
    gy, gx = flow[1], flow[0]
    H, W = gx.shape
    f = np.zeros((H, W))
    f[:-1, 1:] += gx[:-1, 1:] - gx[:-1, :-1]
    f[1:, :-1] += gy[1:, :-1] - gy[:-1, :-1]
    f = f[1:-1, 1:-1]
    t = sf.dst(sf.dst(f, type=2, norm="ortho", axis=1), type=2, norm="ortho", axis=0)
    x, y = np.meshgrid(range(1, W - 1), range(1, H - 1))
    d = (2 * np.cos(np.pi * x / W) - 2) + (2 * np.cos(np.pi * y / H) - 2)
    out = np.zeros((H, W))
    out[1:-1, 1:-1] = sf.idst(sf.idst(t / d, type=2, norm="ortho", axis=1), type=2, norm="ortho", axis=0)
    return out


def host_time(flow, reps):
    host_restatement(flow)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        host_restatement(flow)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def run_bench(args):
    res = {"device": torch.cuda.get_device_name(0), "flop_per_flow": {f"{H}x{W}": flop_per_flow(H, W) for H, W in GEOMETRIES},
           "device_calls": [], "host_restatement": []}
    for H, W in GEOMETRIES:
        for dt in ("float32", "float64"):
            for B in BATCHES:
                flow = torch.from_numpy(synth(B, H, W, dt)).cuda()
                reps = max(3, min(50, int(2e10 / (flop_per_flow(H, W) * B))))
                ms = device_time(flow, reps)
                res["device_calls"].append({"H": H, "W": W, "B": B, "dtype": dt, "ms_per_call": ms, "ms_per_flow": ms / B,
                                            "tflops_from_events": flop_per_flow(H, W) * B / (ms * 1e-3) * 1e-12, "calls": reps})
                print(json.dumps(res["device_calls"][-1]), flush=True)
                del flow
                torch.cuda.empty_cache()
        one = synth(1, H, W, "float64")[0]
        hms = host_time(one, 3 if H * W > 300_000 else 10)
        res["host_restatement"].append({"H": H, "W": W, "ms_per_flow": hms, "threads": torch.get_num_threads()})
        print(json.dumps(res["host_restatement"][-1]), flush=True)
    for r in res["host_restatement"]:
        dev = [d for d in res["device_calls"] if (d["H"], d["W"], d["B"], d["dtype"]) == (r["H"], r["W"], 1, "float64")][0]
        dev8 = [d for d in res["device_calls"] if (d["H"], d["W"], d["B"], d["dtype"]) == (r["H"], r["W"], 8, "float64")][0]
        r["speedup_vs_device_B1"] = r["ms_per_flow"] / dev["ms_per_flow"]
        r["speedup_vs_device_B8_per_flow"] = r["ms_per_flow"] / dev8["ms_per_flow"]
    if args.mfma_json and os.path.exists(args.mfma_json):
        res["mfma_f64"] = json.load(open(args.mfma_json))
    return res


def run_quick():
    (H, W), B, dt, calls = QUICK
    flow = torch.from_numpy(synth(B, H, W, dt)).cuda()
    from event_based_bos_amd.poisson import poisson_reconstruct_batch
    for _ in range(calls):
        poisson_reconstruct_batch(flow)
    torch.cuda.synchronize()
    print(f"[bench_poisson --quick] {calls} calls of {B} x {H} x {W} {dt}")


def merge_stats(args):
    (H, W), B, dt, calls = QUICK
    rows = list(csv.DictReader(open(args.merge_stats)))
    kernels = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "poisson" not in name:
            continue
        kernels[name] = {"calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"]), "avg_ns": float(r["AverageNs"])}
    # (the warm-up-free loop: every call launches each kernel once; per-call time = total / calls of that kernel)
    per_call_ns = sum(k["total_ns"] / k["calls"] for k in kernels.values())
    gemm_ns = sum(k["total_ns"] / k["calls"] for n, k in kernels.items() if "poisson_gemm" in n)
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    q = {"H": H, "W": W, "B": B, "dtype": dt, "kernels": kernels, "kernel_ms_per_call": per_call_ns * 1e-6,
         "kernel_ms_per_flow": per_call_ns * 1e-6 / B, "gemm_ms_per_flow": gemm_ns * 1e-6 / B,
         "tflops_kernel": flop_per_flow(H, W) * B / (per_call_ns * 1e-9) * 1e-12}
    mf = res.get("mfma_f64") or (json.load(open(args.mfma_json)) if args.mfma_json and os.path.exists(args.mfma_json) else None)
    if mf:
        peak = max(mf["chip_tflops_1wave_per_simd"], mf["chip_tflops_2waves_per_simd"])
        q["measured_mfma_f64_tflops"] = peak
        q["share_of_measured_mfma_f64"] = q["tflops_kernel"] / peak
    res["kernel_trace"] = q
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(q, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_bench.json"))
    ap.add_argument("--mfma-json", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats is not None:
        return merge_stats(args)
    if args.quick:
        return run_quick()
    res = run_bench(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
