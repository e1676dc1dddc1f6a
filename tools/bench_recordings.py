#!/usr/bin/env python3
"""Time of the EVT 2.0, EVT 2.1 and DAT decodes (event_based_bos_amd.recordings, csrc/evt2.hip) on the synthetic 1280 x 720 stream
of tools/bench_evt3.py, so that the figures stand beside the EVT 3.0 decoder's.

The stream: that tool's block of bursts (1 to 12 events on one row at one microsecond) over 2^24 us, written by the package's
encoder once and repeated; the decoded times repeat with every copy.  ``evt21-sparse`` is the same block with one event a word
(``vectorize=False``), ``evt21`` packs the bursts into vector words.  Reported, one JSON line per format:
  scan_ms / emit_ms     device events around ebos_evt2_scan (the summary and the scan kernel) and ebos_evt2_emit, slab by slab, median;
                        DAT has no scan pass
  kernels               the kernels' average times, where --kernel-stats names the CSV of a `rocprofv3 --kernel-trace --stats
                        --output-format csv` run of this tool (a run of its own: --device-only --reps 5), or a CSV of the same
                        columns with one row per kernel and grid (profiles/recordings_kernel_stats.csv)
  copy_rate             a device-to-device copy of 1 GiB timed in the same run: bytes read plus bytes written per second
  bytes_must_move       what the decode must move: the words in once, 13 B per event and 10 B per trigger out
  share_of_copy_rate    bytes_must_move / (scan_ms + emit_ms) over copy_rate
  file_to_host_ms       decode_recording: the file read in slabs, decoded, the columns back on the host

    python tools/bench_recordings.py [--format evt2|evt21|evt21-sparse|dat|all] [--events 100000000] [--reps 7] [--device-only]
                                     [--kernel-stats stats.csv] [--json out.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from event_based_bos_amd import recordings  # noqa: E402
from bench_evt3 import H, W, block_columns  # noqa: E402

FORMATS = ("evt2", "evt21", "evt21-sparse", "dat")
KERNELS = ("evt2_summary_kernel", "evt2_scan_kernel", "evt2_emit_kernel", "evt21_emit_kernel", "dat_decode_kernel")


def copy_rate(n_bytes: int = 1 << 30, reps: int = 5) -> float:
    """Bytes read plus bytes written per second of a device-to-device copy of ``n_bytes``, median of ``reps``."""
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda").zero_()
    b = torch.empty_like(a)
    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return 2 * n_bytes / (float(np.median(times)) * 1e-3)


def encode(fmt: str, n_events: int):
    """(one block's words or records, its events, its trigger records)"""
    x, y, t, p, triggers = block_columns(n_events)
    if fmt == "evt2":
        return recordings.encode_evt2(x, y, t, p, triggers), len(t), len(triggers)
    if fmt == "dat":
        return recordings.encode_dat(x, y, t, p).reshape(-1), len(t), 0
    return recordings.encode_evt21(x, y, t, p, triggers, vectorize=fmt == "evt21"), len(t), len(triggers)


def words_times(words: np.ndarray, reps: int, slab_words: int):
    """Median milliseconds of the scan entry and of the emit entry over the whole stream (slab by slab, carry on the device), and
    the totals."""
    signed = np.int32 if words.dtype == np.uint32 else np.int64
    scan_ms, emit_ms = [], []
    n_ev = n_tr = 0
    for r in range(reps + 1):
        carry, s_ms, e_ms, n_ev, n_tr = None, 0.0, 0.0, 0, 0
        for lo in range(0, len(words), slab_words):
            w = torch.from_numpy(words[lo:lo + slab_words].view(signed)).cuda()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            scratch, totals, carry = recordings.evt2_scan(w, carry)
            ev[1].record()
            ne, nt = totals.tolist()
            cols = [torch.empty(ne, dtype=d, device="cuda") for d in (torch.int16, torch.int16, torch.int64, torch.uint8)]
            trig = [torch.empty(nt, dtype=d, device="cuda") for d in (torch.int64, torch.uint8, torch.uint8)]
            ev[2].record()
            recordings.evt2_emit(w, scratch, ne, nt, *cols, *trig)
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


def dat_times(records: np.ndarray, reps: int, slab_words: int):
    from event_based_bos_amd import _hip

    lib = _hip.require_gpu()
    times, n = [], 0
    for r in range(reps + 1):
        ms, n = 0.0, 0
        for lo in range(0, len(records), 2 * slab_words):
            w = torch.from_numpy(records[lo:lo + 2 * slab_words].view(np.int32)).cuda()
            k = w.numel() // 2
            cols = [torch.empty(k, dtype=d, device="cuda") for d in (torch.int16, torch.int16, torch.int64, torch.uint8)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _hip.check(lib.ebos_dat_decode(_hip.ptr(w), k, 2, *(_hip.ptr(c) for c in cols), k, _hip.stream_ptr(w.device)), "ebos_dat_decode")
            e1.record()
            torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
            n += k
            del cols, w
        if r:
            times.append(ms)
    return 0.0, float(np.median(times)), n, 0


def kernel_stats(path: str):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    key = k
                    if row.get("GridX"):     # (one row per grid: the slabs of a stream differ in length)
                        key += " grid " + row["GridX"]
                    out[key] = {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) / 1e6}
    return out


def run(fmt: str, a, rate: float) -> dict:
    one, ev_block, tr_block = encode(fmt, min(a.block_events, a.events))
    copies = -(-a.events // ev_block)
    stream = np.tile(one, copies)
    r = {"format": fmt, "sensor": [H, W]}
    if fmt == "dat":
        scan_ms, emit_ms, n_ev, n_tr = dat_times(stream, a.reps, a.slab_words)
        n_items, item_bytes = len(stream) // 2, 8
    else:
        n_items, item_bytes = len(stream), stream.dtype.itemsize
        r["chunk_words"] = recordings.chunk_words("EVT2" if fmt == "evt2" else "EVT21")
        scan_ms, emit_ms, n_ev, n_tr = words_times(stream, a.reps, a.slab_words)
    assert (n_ev, n_tr) == (copies * ev_block, copies * tr_block), "the decode lost or invented events"
    must = item_bytes * n_items + 13 * n_ev + 10 * n_tr
    seconds = (scan_ms + emit_ms) * 1e-3
    r.update({"events": n_ev, "triggers": n_tr, "words": int(n_items), "word_bytes": item_bytes, "events_per_word": n_ev / n_items,
              "slab_words": a.slab_words, "scan_ms": scan_ms, "emit_ms": emit_ms, "bytes_must_move": must, "GBps": must / seconds / 1e9,
              "copy_rate": rate, "share_of_copy_rate": must / seconds / rate, "events_per_second": n_ev / seconds,
              "device": torch.cuda.get_device_name(0)})
    if a.kernel_stats:
        r["kernels"] = kernel_stats(a.kernel_stats)
    if not a.device_only:
        with tempfile.TemporaryDirectory(prefix="ebos_recordings_") as d:
            if fmt == "dat":
                path = os.path.join(d, "events_td.dat")
                recordings.write_dat_file(path, stream, W, H)
            else:
                path = os.path.join(d, "cd_events.raw")
                recordings.write_raw_file(path, stream, W, H, "EVT2" if fmt == "evt2" else "EVT21")
            times = []
            for k in range(3):
                t0 = time.perf_counter()
                x, y, t, p, triggers, _ = recordings.decode_recording(path, slab_words=a.slab_words)
                times.append((time.perf_counter() - t0) * 1e3)
                assert len(x) == n_ev and len(triggers) == n_tr
                del x, y, t, p
            r["file_bytes"] = os.path.getsize(path)
            r["file_to_host_ms"] = float(np.median(times[1:]))
            r["file_to_host_events_per_second"] = n_ev / (r["file_to_host_ms"] * 1e-3)
    return r


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--format", default="all", choices=FORMATS + ("all",))
    ap.add_argument("--events", type=int, default=100_000_000)
    ap.add_argument("--block-events", type=int, default=12_500_000)
    ap.add_argument("--slab-words", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device-only", action="store_true", help="skip the file: no file_to_host_ms")
    ap.add_argument("--kernel-stats", default=None, help="kernel stats CSV of a rocprofv3 run of this tool")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recordings needs a GPU: a time taken anywhere else says nothing")
    rate = copy_rate()
    results = []
    for fmt in (FORMATS if a.format == "all" else (a.format,)):
        results.append(run(fmt, a, rate))
        print(json.dumps(results[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
