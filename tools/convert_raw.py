#!/usr/bin/env python3
"""Convert a Prophesee EVT 3.0 recording (``cd_events.raw``) into the ``.npz`` of raw columns that ``RawEventStore`` reads, and
optionally its trigger edges into the reference's ``trigger_events.txt`` (whitespace-separated ``t id polarity``).  The stream is
decoded on the GPU (``event_based_bos_amd.evt3``); ``RawEventStore("cd_events.raw")`` reads the same file without this step.

    python tools/convert_raw.py in.raw out.npz [--triggers trigger_events.txt] [--height H --width W]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_bos_amd as ebos  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("raw")
    ap.add_argument("npz")
    ap.add_argument("--triggers", help="also write the trigger records here")
    ap.add_argument("--height", type=int, help="sensor height, for a file whose header holds no geometry")
    ap.add_argument("--width", type=int)
    a = ap.parse_args(argv)
    if (a.height is None) != (a.width is None):
        ap.error("--height and --width come together")
    store = ebos.RawEventStore(a.raw, sensor_size=None if a.height is None else (a.height, a.width))
    c = store.event_data
    ebos.RawEventStore.save(a.npz, c["x"], c["y"], c["t"], c["p"])
    print(f"{a.npz}: {len(store)} events, t {c['t'].dtype}, {store.header.width} x {store.header.height}, "
          f"{store.dropped_outside} outside the geometry dropped, {len(store.triggers)} trigger records")
    if a.triggers:
        np.savetxt(a.triggers, store.triggers, fmt="%d")
    return 0


if __name__ == "__main__":
    sys.exit(main())
