#!/usr/bin/env python3
"""Convert a Prophesee recording -- an EVT 2.0, EVT 2.1 or EVT 3.0 ``.raw`` file or a ``.dat`` file -- into the ``.npz`` of raw
columns that ``RawEventStore`` reads, and optionally its trigger edges into the reference's ``trigger_events.txt``
(whitespace-separated ``t id polarity``); or, with ``--to``, into a recording of another format.  The stream is decoded on the GPU
(``event_based_bos_amd.recordings``); ``RawEventStore("cd_events.raw")`` reads the same file without this step.

    python tools/convert_raw.py in.raw out.npz [--triggers trigger_events.txt] [--height H --width W] [--half-swapped 0|1]
    python tools/convert_raw.py in.raw out.dat --to dat          # or: out.raw --to evt2 | evt21 | evt3

A DAT file holds no triggers, EVT 3.0 trigger ids are 4 bits, and DAT times are 32 bits: what the target cannot hold is refused by
its encoder.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_bos_amd as ebos  # noqa: E402


def write_recording(path: str, fmt: str, store) -> None:
    """The store's events (and, where the format holds them, its trigger records) as a file of format ``fmt``."""
    r, c = ebos.recordings, store.event_data
    x, y, t, p = c["x"], c["y"], c["t"], c["p"]
    width, height = store.header.width, store.header.height
    if fmt == "dat":
        if len(store.triggers):
            print(f"{path}: a DAT file holds no triggers; {len(store.triggers)} trigger records are left out")
        r.write_dat_file(path, r.encode_dat(x, y, t, p), width, height)
    elif fmt == "evt3":
        r.write_raw_file(path, ebos.evt3.encode_evt3(x, y, t, p, store.triggers), width, height, "EVT3")
    else:
        encode = r.encode_evt2 if fmt == "evt2" else r.encode_evt21
        r.write_raw_file(path, encode(x, y, t, p, store.triggers), width, height, fmt.upper())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("raw", help="the recording: .raw (EVT 2.0, 2.1, 3.0) or .dat")
    ap.add_argument("out", help="the .npz of raw columns, or with --to the recording to write")
    ap.add_argument("--to", choices=("evt2", "evt21", "evt3", "dat"), help="write a recording of this format instead of an .npz")
    ap.add_argument("--triggers", help="also write the trigger records here")
    ap.add_argument("--height", type=int, help="sensor height, for a file whose header holds no geometry")
    ap.add_argument("--width", type=int)
    ap.add_argument("--half-swapped", type=int, choices=(0, 1), help="the word order of an EVT 2.1 file, against what its header says")
    a = ap.parse_args(argv)
    if (a.height is None) != (a.width is None):
        ap.error("--height and --width come together")
    store = ebos.RawEventStore(a.raw, sensor_size=None if a.height is None else (a.height, a.width),
                               half_swapped=None if a.half_swapped is None else bool(a.half_swapped))
    c = store.event_data
    if a.to:
        write_recording(a.out, a.to, store)
    else:
        ebos.RawEventStore.save(a.out, c["x"], c["y"], c["t"], c["p"])
    print(f"{a.out}: {len(store)} events from {store.header.format}, t {c['t'].dtype}, {store.header.width} x {store.header.height}, "
          f"{store.dropped_outside} outside the geometry dropped, {len(store.triggers)} trigger records")
    if a.triggers:
        np.savetxt(a.triggers, store.triggers, fmt="%d")
    return 0


if __name__ == "__main__":
    sys.exit(main())
