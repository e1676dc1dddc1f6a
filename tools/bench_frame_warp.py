#!/usr/bin/env python3
"""Timing of the frame warp (event_based_bos_amd/frame_warp.py, csrc/frame_warp.hip).

    python tools/bench_frame_warp.py [--out profiles/frame_warp_bench.json] [--reps 200]
    rocprofv3 --kernel-trace --stats -d <dir> -o fw -- python tools/bench_frame_warp.py --kernels-only --only linear --batch 1
    python tools/bench_frame_warp.py --merge-trace linear=<dir>/fw_results.db [linear_roi=... nearest=... linear_identity=...]

The first line writes the JSON; the second, a run of its own per variant, records the kernel alone; the third reads the kernel
durations out of those runs' databases and adds them to the JSON as its ``kernel_trace`` block (no GPU needed).

The reference's size: a 1200 x 1920 uint8 camera frame into the 720 x 1280 event view, whole and with the YAML's ROI (all rows,
columns 320 .. 960) fused in.

(a) device frames, B in {1, 8, 64}: time per call from device events around a loop of calls (at B = 1 this is the launch rate of
    the Python call, not the kernel: see the rocprofv3 line above for the kernel alone), per frame, and the bytes the warp has to
    move (the source pixels under the destination rectangle, read once, plus the destination written once) over that time as a
    share of the device-to-device copy rate measured in the same run (a 256 MiB copy) -- and, because a 3 MB job cannot reach that
    rate, against a plain copy of the same number of bytes.
(b) what binds: the same launch with INTER_NEAREST (the same coordinate arithmetic, a quarter of the gathers, no blend), with
    float32 frames (four times the bytes), and with the identity matrix (the same arithmetic, perfectly local gathers).
(c) the host: the numpy restatement (tests/_warp_ref.py) on one frame, and ``FrameStore.load_images`` from page-locked frames
    (upload + warp + crop) per frame.
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
import _warp_ref as R  # noqa: E402
from _warp_cases import HOMOGRAPHY, YAML_ROI, textured  # noqa: E402

SRC, DST = (1200, 1920), (720, 1280)
fw = ebos.frame_warp


def source_bytes(M, roi, itemsize):
    """Bytes of the source under the destination rectangle: the bounding box of its four corners, clipped to the frame."""
    xmin, xmax, ymin, ymax = roi
    Mi = np.linalg.inv(M)
    pts = np.array([[ymin, xmin, 1.0], [ymax, xmin, 1.0], [ymin, xmax, 1.0], [ymax, xmax, 1.0]]) @ Mi.T
    xs, ys = pts[:, 0] / pts[:, 2], pts[:, 1] / pts[:, 2]
    w = min(SRC[1], np.ceil(xs.max()) + 1) - max(0, np.floor(xs.min()))
    h = min(SRC[0], np.ceil(ys.max()) + 1) - max(0, np.floor(ys.min()))
    return int(max(w, 0) * max(h, 0)) * itemsize


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
    t = event_time(lambda: b.copy_(a), 20)
    return 2 * a.numel() / t


def device_rows(reps, rate, kernels_only=False, only=None, batch=None):
    rs = np.random.RandomState(0)
    frames = {"uint8": torch.from_numpy(textured(rs, 8, SRC[0], SRC[1], "uint8")).cuda().repeat(8, 1, 1)}
    frames["float32"] = frames["uint8"][:8].float()
    full = (0, DST[0], 0, DST[1])
    variants = [("linear", "uint8", HOMOGRAPHY, fw.INTER_LINEAR, full, (1, 8, 64)), ("linear_roi", "uint8", HOMOGRAPHY, fw.INTER_LINEAR, YAML_ROI, (1, 8, 64)),
                ("nearest", "uint8", HOMOGRAPHY, fw.INTER_NEAREST, full, (8,)), ("linear_f32", "float32", HOMOGRAPHY, fw.INTER_LINEAR, full, (8,)),
                ("linear_identity", "uint8", np.eye(3), fw.INTER_LINEAR, full, (8,))]
    rows = []
    for name, dtype, M, flags, roi, batches in variants:
        if only is not None and name != only:
            continue
        for B in (batches if batch is None else (batch,)):
            src = frames[dtype][:B]
            out = torch.empty((B, roi[1] - roi[0], roi[3] - roi[2]), dtype=src.dtype, device="cuda")
            call = lambda: fw.warp_perspective_batch(src, M, (DST[1], DST[0]), flags, 0, roi, out=out)  # noqa: E731
            if kernels_only:
                for _ in range(reps):
                    call()
                torch.cuda.synchronize()
                continue
            t = event_time(call, reps)
            nbytes = B * (source_bytes(M, roi, src.element_size()) + out[0].numel() * out.element_size())
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            b = torch.empty_like(a)
            t_copy = event_time(lambda: b.copy_(a), reps)
            rows.append({"variant": name, "dtype": dtype, "B": B, "us_per_call": t * 1e6, "us_per_frame": t / B * 1e6, "bytes": nbytes,
                         "GB_per_s": nbytes / t / 1e9, "share_of_measured_copy_rate": nbytes / t / rate,
                         "same_bytes_copy_us": t_copy * 1e6, "time_over_same_bytes_copy": t / t_copy})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def host_rows(reps):
    rs = np.random.RandomState(1)
    frames = textured(rs, 8, SRC[0], SRC[1], "uint8")
    t0 = time.perf_counter()
    for k in range(2):
        R.warp_perspective(frames[k], HOMOGRAPHY, (DST[1], DST[0]))
    host = (time.perf_counter() - t0) / 2
    store = ebos.FrameStore(frames, np.arange(8) * 10_000 + 1_000_000, HOMOGRAPHY, DST).pin()
    common = dict(zip(("xmin", "xmax", "ymin", "ymax"), YAML_ROI))
    t = event_time(lambda: store.load_images(range(8), roi=common), max(10, reps // 10))
    one = event_time(lambda: store.load_images([3], roi=common), max(10, reps // 10))
    return {"numpy_restatement_ms_per_frame": host * 1e3, "load_images_B8_us_per_frame": t / 8 * 1e6, "load_images_B1_us": one * 1e6,
            "note": "load_images: asynchronous upload of the raw 1200 x 1920 frames from page-locked memory + one warp launch with "
                    "the ROI; device-event time, so the upload over the host link is included"}


def merge_trace(out, pairs):
    """``kernel_trace`` of the JSON at ``out``: per variant the durations of the warp kernel's dispatches in a rocprofv3 database."""
    import sqlite3

    res = json.load(open(out))
    block = res.setdefault("kernel_trace", {"source": "rocprofv3 --kernel-trace, one run of --kernels-only --only <variant> --batch 1 per "
                                                      "variant; durations of the warp kernel's dispatches in us (uint8, B = 1)"})
    for pair in pairs:
        variant, path = pair.split("=", 1)
        with sqlite3.connect(path) as db:
            d = np.array([r[0] for r in db.execute("select end - start from kernels where name like '%warp_perspective_kernel%'")]) * 1e-3
        assert d.size, f"{path}: no dispatch of the warp kernel"
        block[variant] = {"dispatches": int(d.size), "median_us": float(np.median(d)), "mean_us": float(d.mean()), "min_us": float(d.min())}
        print(json.dumps({variant: block[variant]}), flush=True)
    json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_warp_bench.json"))
    ap.add_argument("--merge-trace", nargs="+", metavar="VARIANT=DB", default=None,
                    help="add the kernel durations of rocprofv3 databases to the JSON at --out and stop")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true", help="only the (a) and (b) launches, for a rocprofv3 kernel trace")
    ap.add_argument("--only", default=None, help="with --kernels-only: one variant (linear, linear_roi, nearest, linear_f32, linear_identity)")
    ap.add_argument("--batch", type=int, default=None, help="with --kernels-only: one batch size (at most 64; float32: 8)")
    args = ap.parse_args()
    if args.merge_trace:
        merge_trace(args.out, args.merge_trace)
        return
    assert torch.cuda.is_available(), "bench_frame_warp needs a GPU"
    if args.kernels_only:
        device_rows(args.reps, 1.0, kernels_only=True, only=args.only, batch=args.batch)
        return
    rate = copy_rate()
    res = {"device": torch.cuda.get_device_name(0), "source": SRC, "destination": DST, "roi": YAML_ROI,
           "measured_copy_rate_GB_per_s": rate / 1e9}
    print(json.dumps({"measured_copy_rate_GB_per_s": rate / 1e9}), flush=True)
    res["device_frames"] = device_rows(args.reps, rate)
    res["host"] = host_rows(args.reps)
    print(json.dumps(res["host"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
