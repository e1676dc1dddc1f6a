#!/usr/bin/env python3
"""Time of the EVT 3.0 decode (event_based_bos_amd.evt3, csrc/evt3.hip) on a synthetic 1280 x 720 stream of a user's size.

The stream: bursts of 1 to 12 events on one row at one microsecond (what the camera packs into vector words) over 2^24 us, written
by the package's encoder once and repeated -- the 24-bit time wraps at every repetition, so the words of every copy are the same and
the decoded times keep rising.  Reported, as one JSON line:
  scan_ms / emit_ms     device events around ebos_evt3_scan (the summary and the scan kernel) and ebos_evt3_emit, slab by slab, median
  kernels               the three kernels' average times, where --kernel-stats names the CSV of a `rocprofv3 --kernel-trace --stats` run
                        of this tool (a run of its own: --device-only --reps 5)
  bytes_moved           what the algorithm moves: the words twice, 13 B per event, 10 B per trigger
  share_of_copy_rate    bytes_moved / (scan_ms + emit_ms) over the measured 6.29 TB/s copy rate of the MI355X
  file_to_host_ms       decode_raw_file: the file read in slabs, decoded, the columns back on the host

    python tools/bench_evt3.py [--events 100000000] [--reps 7] [--device-only] [--kernel-stats stats.csv] [--json out.json]
"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from event_based_bos_amd import evt3  # noqa: E402

COPY_RATE = 6.29e12   # B/s, the measured device-to-device copy rate
H, W = 720, 1280


def block_columns(n_events: int, seed: int = 0):
    """One repetition as columns: about ``n_events`` events (x, y, t, p) in bursts over [0, 2^24) us, and a trigger edge every 10 ms."""
    rng = np.random.default_rng(seed)
    n_bursts = max(n_events * 2 // 13, 2)
    lens = rng.integers(1, 13, size=n_bursts)
    bt = np.sort(rng.integers(0, 1 << 24, size=n_bursts))
    bt[0], bt[-1] = 0, (1 << 24) - 1            # the first TIME_HIGH of a copy is 0, the last 4095: a wrap between two copies
    owner = np.repeat(np.arange(n_bursts), lens)
    first = np.cumsum(lens) - lens
    step = rng.integers(1, 3, size=len(owner))
    step[first] = 0
    within = np.cumsum(step) - np.repeat(np.cumsum(step)[first], lens)
    x = rng.integers(0, W - 24, size=n_bursts)[owner] + within
    y = rng.integers(0, H, size=n_bursts)[owner]
    p = rng.integers(0, 2, size=n_bursts)[owner]
    stamps = np.arange(5000, 1 << 24, 10_000)
    triggers = np.stack([np.repeat(stamps, 2) + np.tile([0, 100], len(stamps)), np.zeros(2 * len(stamps), np.int64),
                         np.tile([1, 0], len(stamps))], 1)
    return x, y, bt[owner], p, triggers


def block(n_events: int, seed: int = 0):
    """One repetition as EVT 3.0 words, its events and its trigger records."""
    x, y, t, p, triggers = block_columns(n_events, seed)
    return evt3.encode_evt3(x, y, t, p, triggers), len(t), len(triggers)


def device_times(words: np.ndarray, reps: int, slab_words: int):
    """Median milliseconds of the scan entry and of the emit entry over the whole stream (slab by slab, carry on the device), and
    the totals."""
    scan_ms, emit_ms = [], []
    n_ev = n_tr = 0
    for r in range(reps + 1):
        carry, s_ms, e_ms, n_ev, n_tr = None, 0.0, 0.0, 0, 0
        for lo in range(0, len(words), slab_words):
            w = torch.from_numpy(words[lo:lo + slab_words].view(np.int16)).cuda()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            scratch, totals, carry = evt3.evt3_scan(w, carry)
            ev[1].record()
            ne, nt = totals.tolist()
            cols = [torch.empty(ne, dtype=d, device="cuda") for d in (torch.int16, torch.int16, torch.int64, torch.uint8)]
            trig = [torch.empty(nt, dtype=d, device="cuda") for d in (torch.int64, torch.uint8, torch.uint8)]
            ev[2].record()
            evt3.evt3_emit(w, scratch, ne, nt, *cols, *trig)
            ev[3].record()
            torch.cuda.synchronize()
            s_ms += ev[0].elapsed_time(ev[1])
            e_ms += ev[2].elapsed_time(ev[3])
            n_ev += ne
            n_tr += nt
            del cols, trig, w, scratch
        if r:   # (the first pass warms up)
            scan_ms.append(s_ms)
            emit_ms.append(e_ms)
    return float(np.median(scan_ms)), float(np.median(emit_ms)), n_ev, n_tr


def kernel_stats(path: str):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in ("evt3_summary_kernel", "evt3_scan_kernel", "evt3_emit_kernel"):
                if k in name:
                    out[k] = {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) / 1e6}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=100_000_000)
    ap.add_argument("--block-events", type=int, default=12_500_000)
    ap.add_argument("--slab-words", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device-only", action="store_true", help="skip the file: no file_to_host_ms")
    ap.add_argument("--kernel-stats", default=None, help="kernel stats CSV of a rocprofv3 run of this tool")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    one, ev_block, tr_block = block(min(a.block_events, a.events))
    copies = -(-a.events // ev_block)
    words = np.tile(one, copies)
    scan_ms, emit_ms, n_ev, n_tr = device_times(words, a.reps, a.slab_words)
    assert (n_ev, n_tr) == (copies * ev_block, copies * tr_block), "the decode lost or invented events"
    moved = 2 * 2 * len(words) + 13 * n_ev + 10 * n_tr
    r = {"sensor": [H, W], "events": n_ev, "triggers": n_tr, "words": int(len(words)), "words_per_event": len(words) / n_ev,
         "slab_words": a.slab_words, "chunk_words": evt3.chunk_words(), "scan_ms": scan_ms, "emit_ms": emit_ms,
         "bytes_moved": moved, "GBps": moved / ((scan_ms + emit_ms) * 1e-3) / 1e9,
         "share_of_copy_rate": moved / ((scan_ms + emit_ms) * 1e-3) / COPY_RATE,
         "events_per_second": n_ev / ((scan_ms + emit_ms) * 1e-3), "device": torch.cuda.get_device_name(0)}
    if a.kernel_stats:
        r["kernels"] = kernel_stats(a.kernel_stats)
    if not a.device_only:
        with tempfile.TemporaryDirectory(prefix="ebos_evt3_") as d:
            path = os.path.join(d, "cd_events.raw")
            evt3.write_raw_file(path, words, W, H)
            times = []
            for k in range(3):
                t0 = time.perf_counter()
                x, y, t, p, triggers, _ = evt3.decode_raw_file(path, slab_words=a.slab_words)
                times.append((time.perf_counter() - t0) * 1e3)
                assert len(x) == n_ev and len(triggers) == n_tr and bool(np.all(np.diff(t[::1000]) >= 0))
                del x, y, t, p
            r["file_bytes"] = os.path.getsize(path)
            r["file_to_host_ms"] = float(np.median(times[1:]))
            r["file_to_host_events_per_second"] = n_ev / (r["file_to_host_ms"] * 1e-3)
    print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
