#!/usr/bin/env python3
"""Milliseconds per window of the GPU event filters (event_based_bos_amd.event_filters): BAF, HOT and the BAF -> HOT chain
(masks chained on the device, one compaction, one host read-back of the kept count), host + device, synchronised, median of
repetitions after warm-up -- for AoS float64 events and raw sensor columns, on uniform, clustered and hot-pixel windows.
With --pipeline: WindowPipeline per-window time at 346 x 260 with eight windows in flight, filters off and on.

    python tools/bench_event_filter.py [--sizes 100000:260x346,2000000:720x1280,10000000:720x1280] [--pipeline] [--json out.json]
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
from event_based_bos_amd import event_filters as F  # noqa: E402

PARAMS = {"BAF_dt": 0.001, "BAF_ksize": 1, "BAF_num_support_event": 1, "BAF_continuous_update": True, "HOT_thresh": 10}


def timed(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def window(n, H, W, kind, seed=0):
    rs = np.random.RandomState(seed)
    x, y = rs.randint(0, H, n), rs.randint(0, W, n)
    if kind in ("clustered", "hot"):
        m, k = n * 3 // 4, max(H * W // 2000, 8)
        c = rs.randint(0, k, m)
        cx, cy = rs.uniform(0, H, k), rs.uniform(0, W, k)
        x[:m] = np.clip(cx[c] + rs.normal(0, 4, m), 0, H - 1).astype(int)
        y[:m] = np.clip(cy[c] + rs.normal(0, 4, m), 0, W - 1).astype(int)
    if kind == "hot":   # 50 hot pixels with 1 % of the events each
        hp = rs.randint(0, [H, W], (50, 2))
        idx = rs.choice(n, 50 * (n // 100), replace=False)
        x[idx], y[idx] = np.repeat(hp[:, 0], n // 100), np.repeat(hp[:, 1], n // 100)
    t = np.sort(rs.randint(0, 50_000, n)).astype(np.int32)
    return x, y, t, rs.randint(0, 2, n)


def bench_case(n, H, W, kind, source):
    x, y, t, p = window(n, H, W, kind)
    dev = torch.device("cuda")
    if source == "f64":
        ev = torch.from_numpy(np.stack([x, y, t / 1e6, p], 1).astype(np.float64)).to(dev)
        mk = lambda: F._Window(events=ev)  # noqa: E731
        in_bytes = 32
    else:
        raw = tuple(torch.from_numpy(a).to(dev) for a in (y.astype(np.int16), x.astype(np.int16), t, p.astype(np.uint8)))
        mk = lambda: F._Window(raw=raw)  # noqa: E731
        in_bytes = 9

    def one(names):
        def run():
            ch = F._Chain(mk(), (H, W))
            for nm in names:
                if nm == "BAF":
                    ch.baf(PARAMS["BAF_dt"], 1, 1, None)
                else:
                    ch.hot(PARAMS["HOT_thresh"])
            return ch.compact()
        return run

    r = {"events": n, "H": H, "W": W, "window": kind, "source": source}
    r["baf_ms"], r["hot_ms"], r["chain_ms"] = timed(one(["BAF"])), timed(one(["HOT"])), timed(one(["BAF", "HOT"]))
    kept = one(["BAF", "HOT"])().n
    r["kept_fraction"] = kept / n
    # the bytes the BAF grouping must move at least: the window once, keys + indices through three radix passes (read + write),
    # times and prefix maxima, the map; as a fraction of 8 TB/s
    moved = n * (in_bytes + 3 * 16 + 8 * 3) + H * W * (4 + 8)
    r["chain_GBps"] = moved / (r["chain_ms"] * 1e-3) / 1e9
    r["chain_frac_of_hbm_peak"] = r["chain_GBps"] / 8000.0
    return r


def bench_pipeline(filters_on, n_windows=16, n=100_000):
    H, W = 260, 346
    cols = {k: [] for k in "xytp"}
    bounds = [0]
    for k in range(n_windows):
        x, y, t, p = window(n, H, W, "clustered", seed=k)
        cols["x"].append(y.astype(np.int16)); cols["y"].append(x.astype(np.int16))
        cols["t"].append(t.astype(np.int32) + 60_000 * k); cols["p"].append(p.astype(np.uint8))
        bounds.append(bounds[-1] + n)
    store = ebos.data_loader.RawEventStore({k: np.concatenate(v) for k, v in cols.items()})
    windows = [(bounds[k], bounds[k + 1]) for k in range(n_windows)]
    import yaml

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cmax_hot_plate1.yaml")))["solver"]
    cfg.pop("filter", None)
    cfg.update(patch={"size": [20, 26], "sliding_window": [20, 26]}, iwe={"method": "bilinear_vote", "blur_sigma": 0},
               optimizer={"method": "Adam", "n_iter": 600, "parameters": {"lr": 0.2}})
    if filters_on:
        cfg["filter"] = {"filters": ["BAF", "HOT"], "parameters": dict(PARAMS)}
    solver = ebos.solver.collections["contrast_maximization"]((H, W), (H, W), solver_config=cfg)
    pipe = ebos.solver.WindowPipeline(solver)
    ms = timed(lambda: pipe.run(store, windows), reps=3) / n_windows
    return {"pipeline": "346x260", "filters": filters_on, "n_concurrent": pipe.n_concurrent, "ms_per_window": ms,
            "windows": n_windows, "events_per_window": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000:260x346,2000000:720x1280,10000000:720x1280")
    ap.add_argument("--windows", default="uniform,clustered,hot")
    ap.add_argument("--sources", default="f64,raw")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for spec in a.sizes.split(","):
        n, hw = spec.split(":")
        H, W = (int(v) for v in hw.split("x"))
        for kind in a.windows.split(","):
            for src in a.sources.split(","):
                r = bench_case(int(n), H, W, kind, src)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.pipeline:
        for on in (False, True):
            r = bench_pipeline(on)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
