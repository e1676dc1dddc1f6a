"""The cases of tests/_voxel_tile_cases.py, pinned without a GPU, so that a failure of tests/test_gpu_voxel_tiles.py is never a broken
case: the constructed runs hold exactly the events they are named for, no event lies within the margin of a kink at any reference time
its case is run at, a hot pixel's bins reach every register slot of the owner backward's whole-wave walk and one of them first appears
beyond the walk's first 64-event trip, the float64 yardstick's gradient is exactly zero in the bins a constructed pixel holds no event
of, and under the amplitudes of ``SPILL_AMP`` enough events leave every triple's tile + halo window."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxel_tile_cases as V  # noqa: E402
from _voxel_tile_cases import ALL, BMA, CONSTRUCTED, HOT_PIXELS, MAIN, PLAN_TILES, TINY  # noqa: E402

ALL_T = (V.T5,) + V.RUN_T


def run_lengths(ev, shape):
    r, c = V.source_pixels(ev)
    return np.bincount(r * shape[1] + c, minlength=shape[0] * shape[1]).reshape(shape)


def test_geometry_is_the_second_order_sweeps():
    grids = {t: (-(-MAIN[0] // t[0]), -(-MAIN[1] // t[1])) for t in PLAN_TILES}
    assert grids == {(64, 64): (2, 3), (32, 64): (3, 3), (32, 32): (3, 5), (16, 64): (5, 3)}
    assert all(MAIN[0] % t[0] and MAIN[1] % t[1] for t in PLAN_TILES)                  # overhang on both axes
    assert {t[:2] for t in V.BUILT} == set(PLAN_TILES) and set(V.SPILL_AMP) == set(V.BUILT) and len(V.BUILT) == 9
    assert all(TINY[0] < t[0] and TINY[1] < t[1] for t in PLAN_TILES) and min(TINY) > min(h for _, _, h in V.BUILT)


@pytest.mark.parametrize("T", ALL_T)
def test_runs_window_holds_the_constructed_runs(T):
    ev, vx = V.runs_window(T), V.voxel_u(MAIN, T)
    assert ev[0, 2] == 0.0 and ev[-1, 2] == 1.0 and ev[:, 2].min() == 0.0 and ev[:, 2].max() == 1.0
    lengths = run_lengths(ev, MAIN)
    for p, k in CONSTRUCTED.items():
        assert lengths[p] == k, (p, k, lengths[p])
    assert sorted(V.RUN_PIXELS.values()) == [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129]
    # the window is the main window everywhere else (but for the pixels that were cleared)
    other = lengths.copy()
    for p in CONSTRUCTED:
        other[p] = 0
    assert other.max() <= V.OWNER_HOT and (other > V.OWNER_CHUNK).any()                 # no hot pixel but the constructed ones
    assert not V.near_kink(ev, vx, ALL)[1:-1].any()
    assert ((ev[:, 0] % 1.0) > 0).sum() > len(ev) // 3                                  # fractional rows
    for p in CONSTRUCTED:                                                               # shuffled: a run of several events is not in time order
        r, c = V.source_pixels(ev)
        t = ev[(r == p[0]) & (c == p[1]), 2]
        assert len(t) < 7 or (np.diff(t) < 0).any(), p


@pytest.mark.parametrize("T", ALL_T)
def test_hot_pixels_fill_every_slot_of_the_whole_wave_walk(T):
    ev = V.runs_window(T)
    slots = -(-T // V.WAVE)
    assert slots <= V.OWNER_SLOTS
    for p in HOT_PIXELS:
        bins = V.run_bins(ev, p, T)
        assert len(bins) == V.HOT_RUN > V.OWNER_HOT and (np.diff(bins) < 0).any()       # unsorted bins
        assert set(bins >> 6) == set(range(slots)), (p, T)                              # every register slot
        assert len(set(bins & 63)) == min(T, V.WAVE), (p, T)                            # every lane that owns a bin
        if T >= 65:
            # more bins than one 64-event trip holds: in ANY order of the run some bin first appears in a later trip; in input
            # order (which a plan keeps for the events of one pixel where its sort is stable) it does too
            assert len(set(bins)) > V.WAVE
            first = {int(k): int(np.argmax(bins == k)) for k in set(bins)}
            assert max(first.values()) >= V.WAVE
    for p, k in V.RUN_PIXELS.items():
        if k > V.OWNER_HOT and T >= 65:
            assert len(set(V.run_bins(ev, p, T) >> 6)) >= 2, (p, T)                      # the shorter hot runs reach beyond slot 0 too


@pytest.mark.parametrize("tile", PLAN_TILES)
def test_constructed_pixels_sit_where_the_walk_can_go_wrong(tile):
    th, tw = tile
    tiles = {(p[0] // th, p[1] // tw) for p in CONSTRUCTED}
    grid = (-(-MAIN[0] // th), -(-MAIN[1] // tw))
    assert {t[0] for t in tiles} == set(range(grid[0])) and {t[1] for t in tiles} == set(range(grid[1]))   # every tile row and column
    assert len(tiles) >= 6
    assert all(V.pixel_of(V.key_of(p, tile), tile) == p for p in CONSTRUCTED)
    a, b = (V.key_of(p, tile) for p in V.HOT_PAIR)
    assert b == a + 1 and a // V.WAVE == b // V.WAVE                                    # two hot lanes of one wave
    assert V.key_of(V.HOT_LANE0, tile) % V.WAVE == 0                                    # lane 0 of its wave
    corner = V.key_of(V.HOT_CORNER, tile)
    wave = range(corner // V.WAVE * V.WAVE, corner // V.WAVE * V.WAVE + V.WAVE)
    assert any(V.pixel_of(k, tile) is None for k in wave)                               # lanes that own nothing, in the hot wave
    n_keys = grid[0] * grid[1] * th * tw
    assert max(k for k in range(n_keys) if V.pixel_of(k, tile) is not None) == corner   # the last in-image key


@pytest.mark.parametrize("T", ALL_T)
def test_yardstick_is_exactly_zero_in_the_bins_a_constructed_pixel_does_not_hold(T):
    ev, vx = V.runs_window(T), V.voxel_u(MAIN, T)
    mask = V.empty_bins_mask(ev, T)
    _, d_voxel = V.ref_variance_grad(("runs", T), ev, vx)
    _, d_multi = V.ref_mean_variance_grad(("runs", T), ev, vx, V.DIRECTIONS[3])
    for d in (d_voxel, d_multi):
        assert d.shape == (T, 2) + MAIN and np.isfinite(d).all()
        assert (d[:, 0][mask] == 0.0).all() and (d[:, 1][mask] == 0.0).all()
        for p in CONSTRUCTED:
            held = np.unique(V.run_bins(ev, p, T))
            assert np.abs(d[held][:, :, p[0], p[1]]).max() > 0.0, p
    assert mask.any() if T > V.T5 else True                                             # (at T = 5 only the short runs leave bins empty)
    assert mask[:, 3, 7].sum() == T - 1 and mask[:, V.HOT_CORNER[0], V.HOT_CORNER[1]].sum() == T - len(set(V.run_bins(ev, V.HOT_CORNER, T)))


def test_other_windows():
    main = V.main_window()
    assert len(main) == V.N_OF[MAIN] == 30_000 and not V.near_kink(main, V.voxel_u(MAIN), ALL)[1:-1].any()
    assert np.abs(V.voxel_u(MAIN)).max() <= 6.0
    empty = V.empty_tiles_window()
    r, c = V.source_pixels(empty)
    assert not ((r >= 32) & (c >= 64)).any() and empty[0, 2] == 0.0 and empty[-1, 2] == 1.0
    for th, tw in PLAN_TILES:                                                           # whole empty tiles of every shape
        lengths = run_lengths(empty, MAIN)
        sums = [lengths[a:a + th, b:b + tw].sum() for a in range(0, MAIN[0], th) for b in range(0, MAIN[1], tw)]
        assert min(sums) == 0 and max(sums) > 0
    tiny = V.main_window(TINY)
    assert len(tiny) == 600 and not V.near_kink(tiny, V.voxel_u(TINY), ALL)[1:-1].any()
    w0, w1, w2 = V.batch_windows()
    assert w0 is V.runs_window() and len(w1) == 0 and len(w2) == V.BATCH_N2 != len(w0)
    assert not V.near_kink(w2, V.batch_voxels()[2], ALL)[1:-1].any() and not np.array_equal(w2[:100], main[:100])
    lw = V.loop_windows()
    assert len(lw[0]) == 30_000 and lw[1][0, 2] == 0.0 and lw[1][-1, 2] == 1.0 and len(lw[1]) == 2 + len(lw[0][1:-1][::3])


@pytest.mark.parametrize("triple", V.BUILT, ids=lambda t: "x".join(map(str, t)))
def test_spill_condition_holds_for_the_chosen_amplitudes(triple):
    amp = V.SPILL_AMP[triple]
    ev, vx = V.spill_window(amp), V.voxel_u(MAIN, V.T5, amp)
    assert not V.near_kink(ev, vx, ("first",) + BMA)[1:-1].any()
    count = V.events_beyond(ev, vx, triple)
    inside6 = V.events_beyond(V.main_window(), V.voxel_u(MAIN), triple)
    print(f"triple {triple}: amp {amp}: {count} of {len(ev)} events beyond the halo and inside the image (amp 6: {inside6})")
    assert count >= V.SPILL_MIN and inside6 == 0
    for d in V.ALL:                                                                     # amp 6 stays inside every halo at every reference time
        assert V.events_beyond(V.main_window(), V.voxel_u(MAIN), triple, d) == 0, d
