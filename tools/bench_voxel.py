#!/usr/bin/env python3
"""Timing of the event voxel grids (event_based_bos_amd/event_voxel.py, csrc/event_voxel.hip).

    python tools/bench_voxel.py [--out profiles/voxel_bench.json] [--rounds 5] [--reps 20]

Per shape -- 100 k events at 346 x 260 with C = 5, 400 k events at 1280 x 720 with C = 15 -- on integer pixels (what the loaders
emit):

(a) ``create_event_voxel`` and ``generate_discretized_event_volume`` through the kernels, on device tensors, against an eager-torch
    restatement of the same function (the reference's code: eight masked ``put_(accumulate=True)`` passes, two for the volume) on
    the same GPU, in the same process;
(b) B = 8 windows of that size through ``event_voxel_batch`` (one set of launches) against eight eager calls, per window.

Times are device events around a loop of calls, taken in alternating rounds (kernel, eager, kernel, ...); the median over the
rounds and their spread (min, max) are kept.  A difference counts as a gain only where the two [min, max] intervals do not
overlap; ``intervals_overlap`` says so per row.  The kernel calls include the one-flag read-back of the reference-named functions
(a synchronisation per call), the eager ones have none.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_bos_amd as ebos  # noqa: E402
from event_based_bos_amd import event_voxel as V  # noqa: E402

CASES = [{"n": 100_000, "shape": (260, 346), "C": 5}, {"n": 400_000, "shape": (720, 1280), "C": 15}]
B = 8


def eager_voxel(x, y, pol, time, voxel_shape, normalize=False):
    """src/utils/event_utils.py:291-366 restated in eager torch."""
    C, H, W = voxel_shape
    grid = x.new_zeros(voxel_shape, dtype=torch.double)
    t_norm = (C - 1) * (time - time[0]) / (time[-1] - time[0])
    x0, y0, t0 = x.int(), y.int(), t_norm.int()
    for xlim in (x0, x0 + 1):
        for ylim in (y0, y0 + 1):
            for tlim in (t0, t0 + 1):
                mask = (xlim < W) & (xlim >= 0) & (ylim < H) & (ylim >= 0) & (tlim >= 0) & (tlim < C)
                w = pol * (1 - (xlim - x).abs()) * (1 - (ylim - y).abs()) * (1 - (tlim - t_norm).abs())
                index = H * W * tlim.long() + W * ylim.long() + xlim.long()
                grid.put_(index[mask], w[mask], accumulate=True)
    if normalize:
        nz = grid != 0
        mean, std = grid[nz].mean(), grid[nz].std()
        grid[nz] = (grid[nz] - mean) / std
    return grid


def eager_volume(events, vol_size):
    """src/utils/event_utils.py:370-440 restated in eager torch (without the bounds assertions, which read back three flags)."""
    T, X, Y = vol_size
    nb = T // 2
    volume = events.new_zeros(vol_size)
    x, y, t, p = events[:, 0].long(), events[:, 1].long(), events[:, 2], events[:, 3]
    ts = (t - t.min()) * ((nb - 1) / (t.max() - t.min()))
    fl, ce = torch.floor(ts + 1e-8), torch.ceil(ts - 1e-8)
    mul = torch.where(p < 0, nb, 0)
    for tb, w in ((fl.long(), torch.floor(ts) + 1 - ts), (ce.long(), ts - fl)):
        volume.view(-1).put_((X * Y) * (tb + mul) + Y * x + y, w, accumulate=True)
    return volume


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
    (ka, a), (kb, b) = row.items()
    row["intervals_overlap"] = not (a["max"] < b["min"] or b["max"] < a["min"])
    return row


def recording(n, shape, windows, seed=0):
    rs = np.random.RandomState(seed)
    H, W = shape
    m = n * windows
    return {"x": rs.randint(0, W, m).astype(np.int16), "y": rs.randint(0, H, m).astype(np.int16),
            "t": np.cumsum(rs.randint(0, 3, m)).astype(np.int32), "p": rs.randint(0, 2, m).astype(bool)}


def rows(rounds, reps):
    out = []
    for case in CASES:
        n, (H, W), C = case["n"], case["shape"], case["C"]
        store = ebos.RawEventStore(recording(n, (H, W), B))
        ev = torch.from_numpy(store.load_event(0, n)).cuda()
        x, y, pol, t = ev[:, 1].contiguous(), ev[:, 0].contiguous(), (2.0 * ev[:, 3] - 1.0).contiguous(), ev[:, 2].contiguous()
        signed = torch.stack([ev[:, 0], ev[:, 1], ev[:, 2], pol], dim=1).contiguous()
        assert torch.allclose(V.create_event_voxel(x, y, pol, t, (C, H, W)), eager_voxel(x, y, pol, t, (C, H, W)), rtol=0, atol=1e-9)
        assert torch.allclose(V.generate_discretized_event_volume(signed, (2 * C, H, W)), eager_volume(signed, (2 * C, H, W)), rtol=0, atol=1e-9)
        row = {"events": n, "shape": [H, W], "C": C, "unit": "us per call (per window in the batch rows)"}
        row["create_event_voxel"] = compare({"kernel": lambda: V.create_event_voxel(x, y, pol, t, (C, H, W)),
                                             "eager_torch": lambda: eager_voxel(x, y, pol, t, (C, H, W))}, rounds, reps)
        row["create_event_voxel_normalized"] = compare({"kernel": lambda: V.create_event_voxel(x, y, pol, t, (C, H, W), True),
                                                        "eager_torch": lambda: eager_voxel(x, y, pol, t, (C, H, W), True)}, rounds, reps)
        row["generate_discretized_event_volume"] = compare({"kernel": lambda: V.generate_discretized_event_volume(signed, (2 * C, H, W)),
                                                            "eager_torch": lambda: eager_volume(signed, (2 * C, H, W))}, rounds, reps)
        cols = store.load_raw(0, n * B)
        ranges = [(b * n, (b + 1) * n) for b in range(B)]
        win = []
        for a, b in ranges:
            e = torch.from_numpy(store.load_event(a, b)).cuda()
            win.append((e[:, 1].contiguous(), e[:, 0].contiguous(), (2.0 * e[:, 3] - 1.0).contiguous(), e[:, 2].contiguous()))
        row[f"batch_of_{B}"] = compare({"kernel": lambda: V.event_voxel_batch(cols, ranges, C, (H, W)),
                                        "eager_torch": lambda: [eager_voxel(*w, (C, H, W)) for w in win]}, rounds, reps, per=B)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
           "method": "device events around a loop of calls; alternating rounds; median and [min, max] over the rounds"}
    res["rows"] = rows(args.rounds, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
