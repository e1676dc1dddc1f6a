#!/usr/bin/env python3
"""Lens rectification on the GPU at 1280x720: the map build, rectified events per second at 100 k / 2 M / 10 M events, and rectified
frames per second -- DESIGN 4.34.

    python tools/bench_rectify.py [--out profiles/rectify_bench.json] [--repeats 20]

What is compared with what.  Events: ``calibration.rectify_events_raw`` (flag, device-wide scan, scatter: three kernels and the
scan's three) against the same gather, mask and ``cat`` written in eager torch, on the same GPU in the same process, with the same
map (positions and polarity are compared exactly; eager torch multiplies the ticks by 1 / ticks_per_second where the kernel, like
numpy and ``load_event``, divides, so ``t`` may differ in its last bit and its largest relative difference is reported).  Both end
in the one host read-back that returns the number of kept events (the eager version's boolean indexing synchronises by itself).  The kernel's share of the copy rate: the bytes the event path MUST move (13 B of raw columns + a 16 B map entry read,
32 B written per kept event; the scan's traffic is overhead, not counted) over its time, against the rate of a device-to-device
``copy_`` of 256 MiB measured in the same process.  Frames: ``undistort_image_batch`` of 8 uint8 frames against nothing (there is
no eager equivalent of the fixed-point sampling); its figure is frames per second and the share of the copy rate on one read and one
write of every frame.  Times are host clocks around work that ends in a device synchronise, the median of ``--repeats`` runs after
two warm-up runs.  Without a GPU the script fails: nothing here can be measured without one.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_bos_amd as ebos  # noqa: E402

H, W = 720, 1280
K = np.array([[900.0, 0.0, 655.3], [0.0, 905.0, 352.1], [0.0, 0.0, 1.0]])
D = (-0.21, 0.06, 8e-4, -5e-4, -0.008)


def timed(fn, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def eager_rectify(col, row, t, pol, rmap, ticks=1e6):
    """The same result in eager torch: gather, mask, cat."""
    Hs, Ws = rmap.shape[:2]
    c, r = col.long(), row.long()
    inside = (c >= 0) & (c < Ws) & (r >= 0) & (r < Hs)
    pos = rmap[torch.where(inside, r, 0), torch.where(inside, c, 0)]
    keep = inside & (pos[:, 0] >= 0) & (pos[:, 0] < Hs) & (pos[:, 1] >= 0) & (pos[:, 1] < Ws)
    ev = torch.cat([pos, (t.double() / ticks)[:, None], (pol != 0).double()[:, None]], 1)
    return ev[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_bench.json"))
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rectify.py measures on the GPU; there is nothing to measure without one"
    dev = torch.device("cuda")
    res = {"sensor": [H, W], "K": K.tolist(), "D": list(D), "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    # the copy rate of this device, in this process: bytes read + bytes written per second
    a = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    med, _, _ = timed(lambda: b.copy_(a), args.repeats)
    copy_rate = 2 * a.numel() / med
    res["copy_rate_GBps"] = round(copy_rate / 1e9, 1)
    del a, b

    def map_build():
        ebos.CameraCalibration(K, D, (H, W)).rectify_map(dev)
    med, lo, hi = timed(map_build, args.repeats)
    res["map_build"] = {"ms": round(med * 1e3, 4), "ms_min": round(lo * 1e3, 4), "ms_max": round(hi * 1e3, 4), "iterations": 20,
                        "bytes_written": H * W * 16}

    calib = ebos.CameraCalibration(K, D, (H, W))
    rmap = calib.rectify_map(dev)
    res["events"] = {}
    for n in (100_000, 2_000_000, 10_000_000):
        rs = np.random.RandomState(n % 1000)
        cols = (torch.from_numpy(rs.randint(0, W, n).astype(np.int16)).to(dev), torch.from_numpy(rs.randint(0, H, n).astype(np.int16)).to(dev),
                torch.from_numpy(np.sort(rs.randint(0, 500_000, n)).astype(np.int32)).to(dev), torch.from_numpy(rs.randint(0, 2, n).astype(np.uint8)).to(dev))
        got, n_sensor, n_image = ebos.rectify_events_raw(*cols, calib)
        want = eager_rectify(*cols, rmap)
        # positions and polarity are compared exactly; eager torch divides the ticks by multiplying with 1 / ticks_per_second, which
        # differs from the kernel's (and numpy's, and load_event's) true division in the last bit of t
        same = bool(got.shape == want.shape and torch.equal(got[:, [0, 1, 3]], want[:, [0, 1, 3]]))
        t_rel = float(((got[:, 2] - want[:, 2]).abs() / want[:, 2].abs().clamp_min(1e-300)).max()) if same and got.shape[0] else float("nan")
        m = int(got.shape[0])
        k_med, k_lo, k_hi = timed(lambda: ebos.rectify_events_raw(*cols, calib), args.repeats)
        e_med, e_lo, e_hi = timed(lambda: eager_rectify(*cols, rmap), args.repeats)
        must_move = n * (13 + 16) + m * 32
        res["events"][str(n)] = {"kept": m, "outside_image": n_image, "equals_eager_positions_and_polarity": same, "t_max_rel_diff_to_eager": t_rel,
                                 "kernel_ms": round(k_med * 1e3, 4), "kernel_ms_min": round(k_lo * 1e3, 4), "kernel_ms_max": round(k_hi * 1e3, 4),
                                 "eager_ms": round(e_med * 1e3, 4), "eager_ms_min": round(e_lo * 1e3, 4), "eager_ms_max": round(e_hi * 1e3, 4),
                                 "kernel_Mev_per_s": round(n / k_med / 1e6, 1), "eager_Mev_per_s": round(n / e_med / 1e6, 1),
                                 "speedup": round(e_med / k_med, 2), "bytes_must_move": must_move,
                                 "share_of_copy_rate": round(must_move / k_med / copy_rate, 4)}
        del got, want
        print(n, res["events"][str(n)], flush=True)

    B = 8
    frames = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (B, H, W)).astype(np.uint8)).to(dev)
    out = torch.empty_like(frames)
    med, lo, hi = timed(lambda: ebos.undistort_image_batch(frames, calib, out=out), args.repeats)
    res["frames_u8"] = {"batch": B, "ms": round(med * 1e3, 4), "ms_min": round(lo * 1e3, 4), "ms_max": round(hi * 1e3, 4),
                        "frames_per_s": round(B / med, 1), "share_of_copy_rate": round(2 * frames.numel() / med / copy_rate, 4)}
    ff = frames.float()
    outf = torch.empty_like(ff)
    med, lo, hi = timed(lambda: ebos.undistort_image_batch(ff, calib, out=outf), args.repeats)
    res["frames_f32"] = {"batch": B, "ms": round(med * 1e3, 4), "ms_min": round(lo * 1e3, 4), "ms_max": round(hi * 1e3, 4),
                         "frames_per_s": round(B / med, 1), "share_of_copy_rate": round(2 * ff.numel() * 4 / med / copy_rate, 4)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
