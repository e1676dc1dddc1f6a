#!/usr/bin/env python3
"""The two routes of the event -> image vote, timed side by side: ``ops.splat(route="atomic")`` (csrc/splat_kernels.hip, float atomics
on the image) against the ordered route (csrc/splat_ordered.hip: ``ops.SplatIndex.build`` + ``vote``).

    python tools/bench_splat.py [--out profiles/splat_bench.json] [--reps 7] [--quick]

One process, alternating rounds after warm-up, device events around a window of at least ``--window-ms`` of back-to-back calls (host
launch gaps included: what a caller of ``ops`` pays).  Per configuration, in ms per call -- best, median and spread (max - min) over the
rounds:

    atomic          torch.zeros image + ebos_splat_*
    ordered         index build + vote (what ``route="ordered"`` costs for one image)
    ordered_build   the index build alone
    ordered_vote    the vote alone on a reused index (every further image of the same events)

Configurations: 346 x 260 and 1280 x 720; 100 k, 2 M and 10 M events; float32 and float64; unit weight, per-event weight, polarity;
and a batch of 8 x 400 k events.  Events are uniform over the image and one pixel around it, seeded.  The images of the two routes are
compared at every size timed (rel-L2), and two ordered votes must have the same bytes.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_bos_amd as ebos  # noqa: E402
from event_based_bos_amd import _hip, ops  # noqa: E402

IMAGES = ((260, 346), (720, 1280))
COUNTS = (100_000, 2_000_000, 10_000_000)
KINDS = ("unit", "weight", "polarity")
BATCH = (8, 400_000)


def make_events(b, n, h, w, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ev = torch.empty((b, n, 4), dtype=torch.float64, device="cuda")
    ev[..., 0] = torch.rand((b, n), generator=g, device="cuda", dtype=torch.float64) * (h + 1) - 1
    ev[..., 1] = torch.rand((b, n), generator=g, device="cuda", dtype=torch.float64) * (w + 1) - 1
    ev[..., 2] = torch.rand((b, n), generator=g, device="cuda", dtype=torch.float64).sort(dim=1).values
    ev[..., 3] = torch.randint(0, 2, (b, n), generator=g, device="cuda").to(torch.float64)
    wt = (0.5 + torch.rand((b, n), generator=g, device="cuda", dtype=torch.float64)).to(dtype)
    return ev.to(dtype).contiguous(), wt.contiguous()


def window(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def bench(b, n, h, w, dtype, kind, reps, window_ms):
    ev, wt = make_events(b, n, h, w, dtype, seed=b * 1000 + n % 997 + h)
    mode = _hip.SPLAT_POLARITY if kind == "polarity" else _hip.SPLAT_BILINEAR
    weight = wt if kind == "weight" else 1.0
    index = ops.SplatIndex.build(ev, (h, w), polarity=kind == "polarity")
    variants = {
        "atomic": lambda: ops.splat(ev, (h, w), (0, 0), weight, mode),
        "ordered": lambda: ops.splat(ev, (h, w), (0, 0), weight, mode, route="ordered"),
        "ordered_build": lambda: ops.SplatIndex.build(ev, (h, w), polarity=kind == "polarity"),
        "ordered_vote": lambda: index.vote(weight, mode),
    }
    # the same image at the size timed; the ordered one twice with the same bytes
    a, o1, o2, o3 = variants["atomic"](), variants["ordered"](), variants["ordered"](), variants["ordered_vote"]()
    if not (torch.equal(o1, o2) and torch.equal(o1, o3)):
        raise SystemExit(f"bench_splat: two ordered votes differ ({b} x {n}, {h} x {w}, {dtype}, {kind})")
    rel = float(((a.double() - o1.double()).norm() / a.double().norm()).item())
    if not rel < (1e-4 if dtype == torch.float32 else 1e-12):
        raise SystemExit(f"bench_splat: the routes differ by rel-L2 {rel:.3e} ({b} x {n}, {h} x {w}, {dtype}, {kind})")
    del a, o1, o2, o3
    inner = {}
    for name, fn in variants.items():       # warm-up, and the calls a window needs
        fn()
        inner[name] = max(1, min(500, math.ceil(window_ms / max(window(fn, 3), 1e-3))))
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            times[name].append(window(fn, inner[name]))
    res = {"batch": b, "events": n, "image": [h, w], "dtype": str(dtype).replace("torch.", ""), "kind": kind, "reps": reps,
           "rel_l2_between_routes": rel, "index_bytes": int(index.workspace.numel()), "unit": "ms per call (device events, host gaps included)"}
    for name, v in times.items():
        res[name] = {"best": round(min(v), 4), "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4), "calls_per_window": inner[name]}
    res["atomic_gevents_per_s"] = round(b * n / res["atomic"]["best"] / 1e6, 3)
    res["ordered_vote_gevents_per_s"] = round(b * n / res["ordered_vote"]["best"] / 1e6, 3)
    # a difference counts when the intervals [best, best + spread] of the two do not overlap
    lo_a, hi_a = res["atomic"]["best"], res["atomic"]["best"] + res["atomic"]["spread"]
    for name in ("ordered", "ordered_vote"):
        lo, hi = res[name]["best"], res[name]["best"] + res[name]["spread"]
        res[name + "_vs_atomic"] = "faster" if hi < lo_a else ("SLOWER" if lo > hi_a else "intervals overlap")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splat_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--quick", action="store_true", help="100 k events on 346 x 260 only (a rehearsal of the tool)")
    a = ap.parse_args()
    _hip.require_gpu()
    configs = []
    for h, w in IMAGES[:1] if a.quick else IMAGES:
        for n in COUNTS[:1] if a.quick else COUNTS:
            for dtype in (torch.float32, torch.float64):
                configs += [(1, n, h, w, dtype, kind) for kind in KINDS]
        if not a.quick:
            configs += [(BATCH[0], BATCH[1], h, w, dtype, "unit") for dtype in (torch.float32, torch.float64)]
    rows = []
    for cfg in configs:
        rows.append(bench(*cfg, reps=a.reps, window_ms=a.window_ms))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
