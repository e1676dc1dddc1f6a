#!/usr/bin/env python3
"""Wall-clock of EventPlan.build / build_raw per window (host + device, synchronised), after warm-up.

    python tools/bench_plan_build.py [--events 10000000] [--height 720 --width 1280]
    python tools/bench_plan_build.py --batch 8 --events 400000 --height 720 --width 1280 [--out profiles/plan_batch_bench.json]

``--batch K``: K consecutive windows of ``--events`` events of one recording (raw columns on the device), deferred lean builds:
the per-window wall time of K single builds in a loop against ONE ``EventPlan.build_raw_batch`` of the same windows -- same process,
alternating, after warm-up; best, median and spread (max - min) over ``--reps`` rounds of each.

``--time-aware --batch K [--time-bin T]``: the stacked time-aware plan of the K windows -- ``TimeAwarePlanStack.from_raw`` against the
route it replaces (``PreparedWindows.events`` -> ``EventPlan.build(time_bin=T)`` -> ``EventPlan.stack_time_aware``), same process,
alternating rounds after warm-up, timed with device events; best and [min, max] per window over ``--reps`` rounds (5 by default).
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
import event_based_bos_amd as ebos  # noqa: E402


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def bench_batch(a):
    """Loop of deferred single builds against one batched build of the same K windows, alternating in one process."""
    H, W, n, K = a.height, a.width, a.events, a.batch
    rs = np.random.RandomState(0)
    tile = ebos.event_plan.choose_tile((H, W))
    raw = [torch.from_numpy(rs.randint(0, W, n * K).astype(np.int16)).cuda(), torch.from_numpy(rs.randint(0, H, n * K).astype(np.int16)).cuda(),
           torch.from_numpy((np.sort(rs.randint(0, 8333 * K, n * K)) + 10_000_000).astype(np.int32)).cuda(),
           torch.from_numpy(rs.randint(0, 2, n * K).astype(np.uint8)).cuda()]
    ranges = [(k * n, (k + 1) * n) for k in range(K)]
    slices = [tuple(c[b:e] for c in raw) for b, e in ranges]

    def loop():
        return [ebos.EventPlan.build_raw(*sl, (H, W), "first", True, tile=tile, deferred=True, emit="compact") for sl in slices]

    def batch():
        return ebos.EventPlan.build_raw_batch(*raw, ranges, (H, W), "first", True, tile=tile, deferred=True)

    # the same plans, at the sizes timed
    for p1, pb in zip(loop(), batch()):
        used = int(p1.grp_offsets[-1]) * 4
        same = (torch.equal(p1.key_offsets, pb.key_offsets) and torch.equal(p1.grp_offsets, pb.grp_offsets) and
                torch.equal(p1.cpix[:used], pb.cpix[:used]) and torch.equal(p1.cdt[:used].view(torch.int32), pb.cdt[:used].view(torch.int32)) and
                torch.equal(p1.part_table, pb.part_table))
        if not same:
            raise SystemExit("bench_plan_build: the batched plans differ from the single builds")
    for _ in range(3):
        loop(), batch()
    torch.cuda.synchronize()
    times = {"loop": [], "batch": []}
    for _ in range(a.reps):
        for name, fn in (("loop", loop), ("batch", batch)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / K)
    res = {"windows": K, "events_per_window": n, "image": [H, W], "tile": list(tile), "reps": a.reps, "unit": "ms per window (host + device)"}
    for name, v in times.items():
        res[name] = {"best": round(min(v), 4), "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}
    res["gain"] = bool(res["batch"]["best"] < res["loop"]["best"] - res["loop"]["spread"])   # below the loop's best by more than its spread
    res["gain_over_median_spread"] = bool(res["batch"]["best"] < res["loop"]["best"] - (res["loop"]["median"] - res["loop"]["best"]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        rows = json.load(open(a.out)) if os.path.exists(a.out) else []
        rows.append(res)
        json.dump(rows, open(a.out, "w"), indent=1)


def bench_time_aware(a):
    """One batched time-aware build from the raw columns against the window-by-window route, alternating in one process."""
    from event_based_bos_amd.evaluation import PreparedWindows

    H, W, n, K, T = a.height, a.width, a.events, a.batch, a.time_bin
    reps = a.reps if a.reps != 20 else 5
    rs = np.random.RandomState(0)
    tile = (64, 64)
    raw = (torch.from_numpy(rs.randint(0, W, n * K).astype(np.int16)).cuda(), torch.from_numpy(rs.randint(0, H, n * K).astype(np.int16)).cuda(),
           torch.from_numpy((np.sort(rs.randint(0, 8333 * K, n * K)) + 10_000_000).astype(np.int32)).cuda(),
           torch.from_numpy(rs.randint(0, 2, n * K).astype(np.uint8)).cuda())
    ranges = [(k * n, (k + 1) * n) for k in range(K)]
    prepared = PreparedWindows(None, None, None, torch.zeros(K), torch.zeros(K), raw, ranges, None, None, 1e6)

    def parent():
        return ebos.EventPlan.stack_time_aware([ebos.EventPlan.build(prepared.events(b), (H, W), "first", True, tile=tile, emit="full", time_bin=T)
                                                for b in range(K)])

    def new():
        return ebos.TimeAwarePlanStack.from_raw(raw, ranges, (H, W), "first", tile, T)

    old, got = parent(), new()   # the same stack, at the sizes timed (up to the order inside a pixel's run: the offsets and the counts)
    if old.ns != got.ns or not torch.equal(old.key_offsets, got.key_offsets):
        raise SystemExit("bench_plan_build: the stack from the raw columns differs from the window-by-window build")
    for _ in range(2):
        parent(), new()
    torch.cuda.synchronize()
    times = {"parent": [], "from_raw": []}
    for _ in range(reps):
        for name, fn in (("parent", parent), ("from_raw", new)):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / K)
    res = {"time_aware": True, "windows": K, "events_per_window": n, "image": [H, W], "tile": list(tile), "time_bin": T, "reps": reps,
           "unit": "ms per window (device events around the whole build, host gaps included)"}
    for name, v in times.items():
        res[name] = {"best": round(min(v), 4), "min_max": [round(min(v), 4), round(max(v), 4)], "rounds": [round(x, 4) for x in v]}
    lo_p, hi_p = res["parent"]["min_max"]
    lo_n, hi_n = res["from_raw"]["min_max"]
    res["verdict"] = "faster" if hi_n < lo_p else ("SLOWER" if lo_n > hi_p else "intervals overlap: no difference counted")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        rows = json.load(open(a.out)) if os.path.exists(a.out) else []
        rows.append(res)
        json.dump(rows, open(a.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--batch", type=int, default=0, help="K > 0: K windows of --events events, loop of single builds against one batched build")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="--batch: append the result to this JSON list")
    ap.add_argument("--time-aware", action="store_true", help="with --batch: the stacked time-aware plan, from_raw against the window-by-window route")
    ap.add_argument("--time-bin", type=int, default=5, help="--time-aware: the number of time bins T")
    a = ap.parse_args()
    if a.time_aware:
        if a.batch <= 0:
            ap.error("--time-aware needs --batch K")
        return bench_time_aware(a)
    if a.batch > 0:
        return bench_batch(a)
    H, W, n = a.height, a.width, a.events
    rs = np.random.RandomState(0)
    col = rs.randint(0, W, n).astype(np.int16)
    row = rs.randint(0, H, n).astype(np.int16)
    t = np.sort(rs.randint(10_000_000, 10_500_000, n)).astype(np.int32)
    pol = rs.randint(0, 2, n).astype(np.uint8)
    ev64 = np.stack([row, col, t / 1e6, pol], 1)
    g64 = torch.from_numpy(ev64).cuda()
    g32 = g64.float()
    raw = [torch.from_numpy(v).cuda() for v in (col, row, t, pol)]
    res = {"events": n, "image": [H, W]}
    res["build_f64_ms"] = timed(lambda: ebos.EventPlan.build(g64, (H, W), "first", True, tile="auto"))
    res["build_f32_ms"] = timed(lambda: ebos.EventPlan.build(g32, (H, W), "first", True, tile="auto"))
    res["build_raw_ms"] = timed(lambda: ebos.EventPlan.build_raw(*raw, (H, W), "first", True, tile="auto"))
    # lean build (emit="compact": ebos_plan_lean -- compact events + offsets only)
    res["lean_f64_ms"] = timed(lambda: ebos.EventPlan.build(g64, (H, W), "first", True, tile="auto", emit="compact"))
    res["lean_f32_ms"] = timed(lambda: ebos.EventPlan.build(g32, (H, W), "first", True, tile="auto", emit="compact"))
    res["lean_raw_ms"] = timed(lambda: ebos.EventPlan.build_raw(*raw, (H, W), "first", True, tile="auto", emit="compact"))
    res["lean_raw_deferred_ms"] = timed(lambda: ebos.EventPlan.build_raw(*raw, (H, W), "first", True, tile="auto", emit="compact",
                                                                         deferred=True))
    res["soa_only_raw_ms"] = timed(lambda: ebos.EventPlan.build_raw(*raw, (H, W), "first", True, tile=None))
    pin = [torch.from_numpy(v).pin_memory() for v in (col, row, t, pol)]
    res["h2d_raw_ms"] = timed(lambda: [v.to("cuda", non_blocking=True) for v in pin])
    pin64 = torch.from_numpy(ev64).pin_memory()
    res["h2d_f64_ms"] = timed(lambda: pin64.to("cuda", non_blocking=True))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
