#!/usr/bin/env python3
"""Generate tests/golden/golden_rectify.npz by running the REFERENCE's ``undistort_events`` (src/utils/event_utils.py:242-266) on
seeded synthetic events.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rectify.py

Two sets, each run on the float64 events and on their float32 cast:
  lens_*    300 events at 37 x 70 against the maps of case A of tests/_rectify_ref.py (``map_y`` = rectified row, ``map_x`` =
            rectified column of every sensor pixel; barrel: some events leave the image).  The maps are NOT stored: they are
            ``_rectify_ref.rectify_map`` of case A, float64 arithmetic of +, *, / alone, and the generator stores their checksum
            (``lens_map_sum``), which the test compares.  Events on the grid, off the grid, on every border, and with negative
            fractional coordinates in (-1, 0), which truncate to pixel 0.
  small_*   200 events at 8 x 12 against stored float32 maps with values below zero (in (-1, 0) they truncate to 0 and are kept),
            at and beyond ``h`` / ``w``, and with ``h, w`` smaller than the maps.
Stored per set: ``<set>_events`` float64 [n, 4], ``<set>_hw``, and per dtype ``<set>_<f64|f32>_idx`` (the rows the reference kept, in
order) with ``<set>_<f64|f32>_kl`` int32 [m, 2] (its columns 0 and 1); the reference's output is exactly those rows with those two
columns replaced, which the generator asserts.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import _rectify_ref as R  # noqa: E402

OUT = os.path.join(HERE, "golden_rectify.npz")


def main():
    import_reference()
    from src.utils.event_utils import undistort_events

    rs = np.random.RandomState(2718)
    out = {}

    def events_for(n, H, W):
        ev = np.zeros((n, 4))
        ev[:, 0] = rs.randint(0, H, n)
        ev[:, 1] = rs.randint(0, W, n)
        third = n // 3
        ev[third:2 * third, :2] += rs.randint(1, 65536, (third, 2)) / 65536.0                      # off the grid
        edge = np.arange(2 * third, n)
        side = rs.randint(0, 4, len(edge))
        ev[edge, 0] = np.where(side == 0, 0, np.where(side == 1, H - 1, ev[edge, 0]))
        ev[edge, 1] = np.where(side == 2, 0, np.where(side == 3, W - 1, ev[edge, 1]))
        neg = edge[::3]
        ev[neg, 0] = -rs.randint(1, 65536, len(neg)) / 65536.0                                     # (-1, 0): pixel 0
        neg = edge[1::3]
        ev[neg, 1] = -rs.randint(1, 65536, len(neg)) / 65536.0
        ev[:, 2] = np.sort(np.rint(rs.uniform(0, 0.05, n) * 1e6)) / 1e6
        ev[:, 3] = rs.randint(0, 2, n)
        return ev

    def run(name, ev, map_x, map_y, h, w):
        out[f"{name}_events"], out[f"{name}_hw"] = ev, np.array([h, w])
        for tag, dt in (("f64", np.float64), ("f32", np.float32)):
            e = ev.astype(dt)
            got = undistort_events(e, map_x, map_y, h, w)
            assert got.dtype == dt
            k = np.int32(map_y[e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)])
            l = np.int32(map_x[e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)])  # noqa: E741
            idx = np.flatnonzero((0 <= k) & (k < h) & (0 <= l) & (l < w)).astype(np.int32)
            want = e[idx].copy()
            want[:, 0], want[:, 1] = k[idx], l[idx]
            assert np.array_equal(got, want), "the reference's output is not the kept rows with columns 0 and 1 replaced"
            assert np.array_equal(got, R.undistort_events(e, map_x, map_y, h, w)), "the restatement differs from the reference"
            out[f"{name}_{tag}_idx"], out[f"{name}_{tag}_kl"] = idx, np.stack([k[idx], l[idx]], 1).astype(np.int32)
            print(f"{name} {tag}: {len(e)} events, {len(idx)} kept")

    H, W = R.CASES["A"]["size"]
    rmap = R.rectify_map(R.case_K("A"), R.CASES["A"]["D"], (H, W))
    out["lens_map_sum"] = np.array([rmap[..., 0].sum(), rmap[..., 1].sum()])
    run("lens", events_for(300, H, W), np.ascontiguousarray(rmap[..., 1]), np.ascontiguousarray(rmap[..., 0]), H, W)

    h, w = 8, 12
    g = R.pixel_grid(h, w)
    map_y = (g[..., 0] + rs.uniform(-2.5, 2.5, (h, w))).astype(np.float32)
    map_x = (g[..., 1] + rs.uniform(-2.5, 2.5, (h, w))).astype(np.float32)
    map_y[0, :4] = [-0.25, -0.999, -1.0, 6.0]
    map_x[0, :4] = [-0.5, 0.999, 3.0, 9.999]
    out["small_map_x"], out["small_map_y"] = map_x, map_y
    run("small", events_for(200, h, w), map_x, map_y, h - 2, w - 2)

    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
