#!/usr/bin/env python3
"""Benchmark of the generative solver's iteration (csrc/gml.hip) against the same objective as eager torch (tests/_gml_ref.py) on the
same GPU and on the CPU.

    python tools/bench_gml.py --out profiles/gml_bench.json

Per size (720 x 1280 and 260 x 346, the reference YAML's options, ROI = the YAML's column band scaled to the width):
  hip_ms_per_iter       ebos_gml_solve_scale_f64 at the finest scale (patch 8), device events around `iters` iterations;
  hip_window_ms         one GenerativePatchPyramid.estimate with n_iter 600 (770 iterations), host clock around a synchronised call;
  torch_gpu_ms_per_iter _gml_ref.Model forward + backward + torch.optim.Adam step on the GPU, float64;
  torch_cpu_ms_per_iter the same on the CPU (a few iterations);
  bytes_per_iter        the float64 traffic the seven passes need at the pixel level (formula below), and its rate against
                        the rate of a device-to-device copy of 256 MiB measured in the same run.

With ``--method patch_eklt_dependent``, the single-scale solver (GenerativePatchDependent) with the YAML's patch_eklt block
(patch 4, slide 2) and the YAML's ROI (the central half of the columns):
  hip_window_ms         one estimate with n_iter 600, host clock around a synchronised call (best of 3);
  hip_ms_per_iter       (window at n_iter 600 - window at n_iter 100) / 500;
  torch_gpu_ms_per_iter _gml_dep_ref.Model forward + backward + torch.optim.Adam step on the GPU, float64 (eager baseline);
  torch_gpu_window_ms   the same iteration times 600.

With ``--batch B [B ...]`` (either method), only the window axis is measured, at n_iter 600 and both sizes:
  sequential_window_ms  one ``estimate`` per window, host clock around a synchronised call (every repeat is kept: their spread is
                        the margin a comparison has to clear);
  batch[B].window_ms    ``estimate_batch`` of B windows (different event counts), divided by B; .ms_per_iter divides by the
                        window's iterations as well.
The kernel table of a batch comes from a run of its own: rocprofv3 --kernel-trace --stats -- python tools/run_gml.py --batch B.
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

import _gml_dep_ref as D  # noqa: E402
import _gml_ref as R  # noqa: E402
from _gml_cases import YAML_COST, YAML_GML, frame_image, synth_events  # noqa: E402

# bytes per pixel and iteration, float64: pass A reads gx, gy (warped: ~1 line each from cache), winv, writes P0 (+ we when set);
# pass B reads P0, q; pass D reads gx, gy, P0, q, winv, writes dF (2), dT (2); pass E reads dF, dT.
BYTES_PER_PIXEL = 8 * ((2 + 1 + 1) + 2 + (2 + 1 + 1 + 1 + 4) + 4)


def config(H, W, n_iter):
    y0, y1 = W // 4, W - W // 4
    return {"method": "patch_eklt_pyramid2", "filter": {"filters": [], "parameters": {"xmin": 0, "xmax": H, "ymin": y0, "ymax": y1}},
            "cost_with_weight": dict(YAML_COST), "optimizer": {"method": "Adam", "n_iter": n_iter}, "generative_ml": dict(YAML_GML)}


def copy_rate():
    a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2 * a.numel() * 20 / (e0.elapsed_time(e1) * 1e-3)   # read + write bytes / s


def bench_size(H, W, iters, cpu_iters):
    import event_based_bos_amd as ebos
    frame, events = frame_image(H, W, 1), synth_events(2 * H * W, H, W, 2)
    out = {"size": [H, W]}
    # one window (770 iterations)
    solv = ebos.solver.GenerativePatchPyramid((H, W), (H, W), {}, config(H, W, 600))
    np.random.seed(0)
    solv.estimate(events, frame=frame)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        np.random.seed(0)
        t0 = time.perf_counter()
        solv.estimate(events, frame=frame)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    out["hip_window_ms"] = 1e3 * min(ts)
    out["hip_window_ms_all"] = [1e3 * t for t in ts]
    # the finest scale's iteration alone
    lib = ebos._hip.require_gpu()
    dev = torch.device("cuda:0")
    cfg = config(H, W, 600)
    roi = tuple(cfg["filter"]["parameters"][k] for k in ("xmin", "xmax", "ymin", "ymax"))
    st = R.prepare(frame, R.polarity_image(events, (H, W)), YAML_GML, roi)
    q = R.measured(st)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gx, gy, qq, wi = t(st["gx"]), t(st["gy"]), t(q), t(st["winv"])
    gh, gw = R.grid_shape(H, W, 8)
    x = t(np.random.RandomState(0).uniform(-1, 1, (3, gh, gw)) * np.array([1, 0.3, 0.3])[:, None, None])
    w = torch.tensor([1.0, 0.5, 0.1], dtype=torch.float64, device=dev)
    o = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    nbytes = int(lib.ebos_gml_scratch_bytes(H, W, 8))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    hist = torch.empty(iters, 4, dtype=torch.float64, device=dev)
    p_ = ebos._hip.ptr

    def run(n):
        ebos._hip.check(lib.ebos_gml_solve_scale_f64(H, W, 8, 3, *roi, 0, p_(w), p_(o), 3, p_(gx), p_(gy), p_(qq), None, p_(wi), p_(x),
                                                     n, 0.05, p_(hist), None, p_(scratch), nbytes, ebos._hip.stream_ptr()), "solve")
    run(10)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(iters)
    e1.record()
    torch.cuda.synchronize()
    out["hip_ms_per_iter"] = e0.elapsed_time(e1) / iters
    out["bytes_per_iter"] = BYTES_PER_PIXEL * H * W
    # eager torch, GPU and CPU
    for name, device, n in (("torch_gpu", "cuda", 20), ("torch_cpu", "cpu", cpu_iters)):
        model = R.Model(st, YAML_GML, YAML_COST, 8, q, device)
        xt = x.detach().to(device).clone().requires_grad_()
        opt = torch.optim.Adam([xt], lr=0.05)

        def step():
            opt.zero_grad()
            loss, _ = model.parts(xt)
            loss.backward()
            opt.step()
        step()
        if device == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        if device == "cuda":
            torch.cuda.synchronize()
        out[name + "_ms_per_iter"] = 1e3 * (time.perf_counter() - t0) / n
    return out


def dep_config(H, W, n_iter):
    cfg = config(H, W, n_iter)
    cfg["method"] = "patch_eklt_dependent"
    cfg["patch_eklt"] = {"patch_size": 4, "sliding_window": 2, "do_event_thresholding": False, "event_thres": 8}
    return cfg


def bench_dep_size(H, W):
    import event_based_bos_amd as ebos
    frame, events = frame_image(H, W, 1), synth_events(2 * H * W, H, W, 2)
    out = {"method": "patch_eklt_dependent", "size": [H, W]}

    def window(n_iter, reps=3):
        solv = ebos.solver.GenerativePatchDependent((H, W), (H, W), {}, dep_config(H, W, n_iter))
        np.random.seed(0)
        solv.estimate(events, frame=frame)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            np.random.seed(0)
            t0 = time.perf_counter()
            solv.estimate(events, frame=frame)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return solv, [1e3 * t for t in ts]

    solv, t600 = window(600)
    _, t100 = window(100)
    out["hip_window_ms"] = min(t600)
    out["hip_window_ms_all"] = t600
    out["hip_window_ms_n100"] = min(t100)
    out["hip_ms_per_iter"] = (min(t600) - min(t100)) / 500
    out["selected_patches"] = int(len(solv.estimate_indices))
    out["grid"] = list(solv.patch_image_size)
    cfg = dep_config(H, W, 600)
    roi = tuple(cfg["filter"]["parameters"][k] for k in ("xmin", "xmax", "ymin", "ymax"))
    st = R.prepare(frame, R.polarity_image(events, (H, W)), YAML_GML, roi)
    idx = solv.estimate_indices
    model = D.Model(st, YAML_GML, YAML_COST, 4, 2, roi, idx, "cuda")
    xt = model.from_grid(solv.params).clone().requires_grad_()
    opt = torch.optim.Adam([xt], lr=0.05)

    def step():
        opt.zero_grad()
        loss, _ = model.parts(xt)
        loss.backward()
        opt.step()
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    out["torch_gpu_ms_per_iter"] = 1e3 * (time.perf_counter() - t0) / 10
    out["torch_gpu_window_ms"] = 600 * out["torch_gpu_ms_per_iter"]
    out["speedup_vs_torch_gpu"] = out["torch_gpu_ms_per_iter"] / out["hip_ms_per_iter"]
    return out


def batch_windows(H, W, n):
    """n windows over one frame: different seeds, different event counts (2 per pixel, down to ~1.5)."""
    return frame_image(H, W, 1), [synth_events(2 * H * W - (i % 4) * (H * W // 6), H, W, 2 + i) for i in range(n)]


def bench_batch_size(method, H, W, batches, reps=3, n_iter=600):
    import event_based_bos_amd as ebos
    dep = method == "patch_eklt_dependent"
    cls = ebos.solver.GenerativePatchDependent if dep else ebos.solver.GenerativePatchPyramid
    solv = cls((H, W), (H, W), {}, (dep_config if dep else config)(H, W, n_iter))
    frame, windows = batch_windows(H, W, max(batches))
    iters = n_iter if dep else sum(n_iter // (5 - s + 1) for s in range(1, 5))
    out = {"method": method, "size": [H, W], "iterations": iters, "batch": {}}

    def timed(fn, n):
        np.random.seed(0)
        fn()   # warm-up: code objects, allocations
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            np.random.seed(0)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts

    seq = timed(lambda: solv.estimate(windows[0], frame=frame), max(reps, 5))
    out["sequential_window_ms"] = min(seq)
    out["sequential_window_ms_all"] = seq
    for b in batches:
        ts = [t / b for t in timed(lambda: solv.estimate_batch(windows[:b], frames=frame), reps)]
        out["batch"][str(b)] = {"window_ms": min(ts), "window_ms_all": ts, "ms_per_iter": min(ts) / iters,
                                "vs_sequential": min(seq) / min(ts)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--method", default="patch_eklt_pyramid2", choices=("patch_eklt_pyramid2", "patch_eklt_dependent"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=None, metavar="B",
                    help="measure estimate_batch at these batch sizes beside the sequential window (nothing else)")
    ap.add_argument("--sizes", type=int, nargs="+", default=(720, 1280, 260, 346), metavar="N", help="--batch: H W [H W ...]")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gml.py measures on the GPU"
    if args.batch:
        res = {"sizes": []}
        for H, W in zip(args.sizes[0::2], args.sizes[1::2]):
            r = bench_batch_size(args.method, H, W, sorted(set(args.batch)), args.reps)
            res["sizes"].append(r)
            print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    if args.method == "patch_eklt_dependent":
        res = {"sizes": []}
        for H, W in ((720, 1280), (260, 346)):
            r = bench_dep_size(H, W)
            res["sizes"].append(r)
            print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    rate = copy_rate()
    res = {"copy_bytes_per_s": rate, "sizes": []}
    for (H, W), cpu_iters in (((720, 1280), 2), ((260, 346), 5)):
        r = bench_size(H, W, args.iters, cpu_iters)
        r["bytes_rate_vs_copy"] = r["bytes_per_iter"] / (r["hip_ms_per_iter"] * 1e-3) / rate
        r["speedup_vs_torch_gpu"] = r["torch_gpu_ms_per_iter"] / r["hip_ms_per_iter"]
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
