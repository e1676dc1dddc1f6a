"""The lean plan build (``ebos_plan_lean``, ``emit="compact"``) on windows with a GIANT pixel run: a stuck pixel that fires more often
in one window than the bin sort's whole LDS staging area holds.  Such a run goes straight to its slots of ``cdt`` and is sorted there
(plan_lean.hip, the ``direct`` branch of ``lean_bin_sort_body``); the contract is the one of every other run: ascending dt inside the
pixel, so two builds of one window hold identical arrays and two solves of it identical trajectories.

Run lengths, from the layout arithmetic (``lean_sort_caps``: LDS of 158 KiB less 8 B per pixel of a row band, 12 B per staged event of
ONE of the two staging buffers; an overfull bin re-stages chunks of whole pixels in both: 2 x sort_cap events):

  * 2 x sort_cap lies between 21 416 (tile 64 x 64, one band: (161 792 - 8 x 65 x 64) / 12 = 10 708 per buffer) and 26 880 (the smallest
    band: no pixels at all) for every built geometry.  On the sensor of this file -- 128 x 128, tile (64, 64), four tiles -- a window of
    up to 141 345 events keeps one band per tile (21 416); the windows of 150 000 to 250 000 events are cut into two bands of 32 rows
    (2 x 12 074 = 24 148).
  * 20 000 is INSIDE the staging area under every layout: the chunked route of an overfull bin, the run sorted in LDS as a hot pixel.
  * 30 000 is BEYOND it under every layout and fits one load of the staging area as floats (3 x sort_cap >= 32 124): direct, one sort.
  * 100 000 needs the odd-even merge-split, over chunks of the largest power of two of which the staging area holds a pair: 7 chunks
    of 16 384 with two bands, 13 of 8 192 with one.

Expected arrays: a plain numpy restatement of the layout from the events themselves (not the full build) -- ``key_offsets`` the counts
of the tile-major pixel key, ``grp_offsets`` the tiles' counts in groups of four, ``cpix`` = (row in tile << 8) | column in tile, ``cdt``
the float32 of the oracle's fp64 ``delta_t``, ascending inside every pixel, NaN / pixel 0 in the padding slots.  Everything is compared
bit for bit."""
import numpy as np
import pytest
import torch

from oracle import ebos_oracle as O

pytestmark = pytest.mark.gpu

SIZE, TILE = (128, 128), (64, 64)
TICKS = 1e6        # ticks per second of the raw columns (RawEventStore.TICKS_PER_SECOND)
WIDE0 = 1 << 33    # first tick of the 64-bit recordings: beyond 2^31
SOURCES = ("aos_f64", "aos_f32", "raw32", "raw64")


def _columns(n, hot, seed, pad_last_tile=False):
    """rows, cols, ticks (int64, stably sorted) of a window of ``n`` events: uniform over the sensor, ``hot`` = ((row, col, count), ...)
    pixels that fire ``count`` times at random places of the window.  Timestamps uniform on [0, 0.5] s in microsecond ticks, a third
    of them rounded to 1e-3 s: every long run holds ties."""
    H, W = SIZE
    rs = np.random.RandomState(seed)
    r, c = rs.randint(0, H, n), rs.randint(0, W, n)
    where = rs.permutation(n)
    at = 0
    for hr, hc, _ in hot:   # (the uniform events stay off the hot pixels: a run is exactly its count)
        c[(r == hr) & (c == hc)] = (hc + 2) % W
    for hr, hc, k in hot:
        r[where[at:at + k]], c[where[at:at + k]] = hr, hc
        at += k
    if pad_last_tile:   # the last tile's events are no multiple of four: NaN padding follows its last run
        last = (r >= H - TILE[0]) & (c >= W - TILE[1])
        if last.sum() % 4 == 0:
            i = np.flatnonzero(last & ~((r == H - 1) & (c == W - 1)))[0]
            r[i], c[i] = 0, 0
    t = rs.randint(0, 500_001, n).astype(np.int64)
    third = rs.randint(0, 3, n) == 0
    t[third] = (t[third] + 500) // 1000 * 1000
    return r, c, np.sort(t, kind="stable")


def _sort_key(dt32):
    """plan_lean.hip's ``sort_key``: a float's bits as an integer with the floats' order (a total order)."""
    b = dt32.view(np.int32)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def _reference(ev64, direction="first", normalize=True):
    """(key_offsets, grp_offsets, cpix, cdt bits, live) of float64 events [n, 4] = (row, col, t in seconds, p), all inside the sensor."""
    (H, W), (th, tw) = SIZE, TILE
    tiles_y, tiles_x = -(-H // th), -(-W // tw)
    n_tiles = tiles_y * tiles_x
    r, c = ev64[:, 0].astype(np.int64), ev64[:, 1].astype(np.int64)
    tile = (r // th) * tiles_x + c // tw
    key = tile * (th * tw) + (r % th) * tw + c % tw
    dt = O.delta_t(ev64, O.reference_time(ev64, direction), normalize).astype(np.float32)
    order = np.lexsort((_sort_key(dt), key))
    key_offsets = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_tiles * th * tw))]).astype(np.int32)
    per_tile = np.bincount(tile, minlength=n_tiles)
    grp_offsets = np.concatenate([[0], np.cumsum((per_tile + 3) // 4)]).astype(np.int32)
    used = 4 * int(grp_offsets[-1])
    cpix = np.zeros(used, np.int16)
    cdt = np.full(used, np.nan, np.float32)
    live = np.zeros(used, bool)
    first = np.concatenate([[0], np.cumsum(per_tile)])
    slot = 4 * grp_offsets[tile[order]].astype(np.int64) + (np.arange(len(order)) - first[tile[order]])
    cpix[slot] = (((r % th) << 8) | (c % tw))[order]
    cdt[slot] = dt[order]
    live[slot] = True
    return key_offsets, grp_offsets, cpix, cdt.view(np.int32), live


def _events_f64(r, c, t):
    return np.stack([r.astype(np.float64), c.astype(np.float64), t / TICKS, np.zeros(len(t))], 1)


def _store(r, c, t):
    import event_based_bos_amd as ebos

    return ebos.data_loader.RawEventStore({"x": c.astype(np.int16), "y": r.astype(np.int16), "t": t, "p": np.zeros(len(t), bool)})


def _source(source, r, c, t):
    """(build(direction, normalize, deferred) -> plan, the float64 events that source stands for)."""
    import event_based_bos_amd as ebos

    if source in ("aos_f64", "aos_f32"):
        ev = _events_f64(r, c, t)
        if source == "aos_f32":
            ev = ev.astype(np.float32)
        dev = torch.from_numpy(ev).cuda()
        return (lambda d="first", nrm=True: ebos.EventPlan.build(dev, SIZE, d, nrm, tile=TILE, emit="compact")), ev.astype(np.float64)
    store = _store(r, c, t.astype(np.int32) if source == "raw32" else t + WIDE0)
    assert store.event_data["t"].dtype == (np.int32 if source == "raw32" else np.int64)
    n = len(t)
    return (lambda d="first", nrm=True, deferred=False: store.plan(0, n, SIZE, d, nrm, tile=TILE, deferred=deferred, emit="compact")), \
        store.load_event(0, n)


def _arrays(plan):
    assert plan.lean and plan.compact and plan.tile == TILE
    used = 4 * int(plan.grp_offsets[-1])
    return (plan.key_offsets.cpu().numpy(), plan.grp_offsets.cpu().numpy(), plan.cpix[:used].cpu().numpy(),
            plan.cdt[:used].view(torch.int32).cpu().numpy())


def _assert_reference(got, ref, what):
    ko, grp, cpix, cdt = got
    rko, rgrp, rcpix, rcdt, live = ref
    np.testing.assert_array_equal(ko, rko, err_msg=f"{what}: key_offsets")
    np.testing.assert_array_equal(grp, rgrp, err_msg=f"{what}: grp_offsets")
    np.testing.assert_array_equal(cpix, rcpix, err_msg=f"{what}: cpix")           # (padding: pixel 0)
    np.testing.assert_array_equal(cdt[live], rcdt[live], err_msg=f"{what}: cdt")  # bits
    assert np.isnan(cdt[~live].view(np.float32)).all(), f"{what}: padding slots hold NaN"


def _assert_same(a, b, what):
    for x, y, name in zip(a, b, ("key_offsets", "grp_offsets", "cpix", "cdt")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


_CACHE = {}


def _window(n, hot, seed, pad_last_tile=False):
    key = (n, hot, seed, pad_last_tile)
    if key not in _CACHE:
        cols = _columns(n, hot, seed, pad_last_tile)
        for a in cols:
            a.setflags(write=False)
        _CACHE[key] = cols
    return _CACHE[key]


def _giant_window(run):
    """The window of the file: a pixel of tile 2 firing ``run`` times among 150 000 events (200 000 around a 100 000 run)."""
    return _window(200_000 if run > 50_000 else 150_000, ((70, 9, run),), seed=31)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("run", [20_000, 30_000, 100_000])
def test_giant_run_is_canonical(run, source):
    """Three builds of the window hold identical arrays, and they are the numpy reference's: 20 000 (inside the staging area: the
    chunked route), 30 000 (direct, one sort in LDS), 100 000 (direct, merge-split), from float64 / float32 events and raw columns with
    4- and 8-byte ticks (the two stamp widths of the direct branch's gather; the 8-byte recording starts beyond 2^31 ticks)."""
    r, c, t = _giant_window(run)
    build, ev64 = _source(source, r, c, t)
    got = [_arrays(build()) for _ in range(3)]
    assert np.diff(got[0][0]).max() == run
    _assert_same(got[0], got[1], "second build")
    _assert_same(got[0], got[2], "third build")
    _assert_reference(got[0], _reference(ev64), (run, source))


POSITIONS = {
    # pixel (0, 0) of a tile: the first chunk of the bin's pixels is the direct one
    "first_pixel_of_a_tile": (150_000, ((0, 64, 30_000),), False),
    # the last pixel of the last tile: the run ends the segment (c1 = len), the tile's NaN padding follows it
    "last_pixel_of_the_last_tile": (150_000, ((127, 127, 30_000),), True),
    # 250 000 events: lean_layout cuts the tiles into two bands of 32 rows (module docstring; the plan does not show its bands) --
    # row 31 of tile 2 ends band 0
    "last_pixel_of_a_row_band": (250_000, ((64 + 31, 63, 30_000),), False),
    "two_giant_pixels_in_one_tile": (150_000, ((5, 70, 30_000), (20, 100, 30_000)), False),
    # the neighbour's 5 000 events take the whole-workgroup network in the chunk that follows the direct one
    "giant_next_to_a_hot_pixel": (150_000, ((70, 9, 30_000), (70, 10, 5_000)), False),
    "every_event_at_one_pixel": (30_000, ((70, 9, 30_000),), False),
}


@pytest.mark.parametrize("case", list(POSITIONS))
def test_giant_run_positions(case):
    """A 30 000-event run at the places where the chunk walk of an overfull bin has an edge: against the reference and against a
    second build."""
    n, hot, pad = POSITIONS[case]
    r, c, t = _window(n, hot, seed=32, pad_last_tile=pad)
    build, ev64 = _source("aos_f64", r, c, t)
    got, again = _arrays(build()), _arrays(build())
    runs = np.sort(np.diff(got[0]))[::-1]
    assert runs[0] == 30_000 and (len(hot) < 2 or runs[1] == hot[1][2])
    if pad:
        assert got[0][-1] < 4 * int(got[1][-1])   # padding slots behind the last run
    _assert_same(got, again, case)
    _assert_reference(got, _reference(ev64), case)


@pytest.mark.parametrize("n,run", [(100_000, 32_124), (100_000, 32_125), (120_000, 100_000), (150_000, 36_222), (150_000, 36_223),
                                   (150_000, 60_000)])
def test_one_load_and_merge_split_boundaries(n, run):
    """The sizes at which the sort of a direct run changes its route: the last run that is one load of the staging area and the first
    that is split, with one band per tile (a window of up to 141 345 events: 3 x 10 708 = 32 124 floats, chunks of 8 192) and with two
    (3 x 12 074 = 36 222, chunks of 16 384); an odd number of chunks (100 000 = 13 of 8 192; 36 223 = 3 of 16 384), whose last one has
    no partner in the first phase, and an even one (60 000 = 4 of 16 384)."""
    r, c, t = _window(n, ((70, 9, run),), seed=34)
    build, ev64 = _source("aos_f64", r, c, t)
    got, again = _arrays(build()), _arrays(build())
    assert np.diff(got[0]).max() == run
    _assert_same(got, again, (n, run))
    _assert_reference(got, _reference(ev64), (n, run))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("direction", ["first", "middle", "last", 0.25])
def test_directions_and_normalisation(direction, normalize):
    """dt of either sign (the sort key's two halves) and in seconds or fractions of the window."""
    r, c, t = _giant_window(30_000)
    build, ev64 = _source("aos_f64", r, c, t)
    got = _arrays(build(direction, normalize))
    assert np.diff(got[0]).max() == 30_000
    _assert_reference(got, _reference(ev64, direction, normalize), (direction, normalize))


def test_batched_build_equals_the_single_builds():
    """``EventPlan.build_raw_batch`` (one ``ebos_plan_lean_batch`` call) on three windows of one recording -- an ordinary one, one with
    a 30 000 run, one with a 100 000 run --: every window's arrays are the single build's, and the reference's."""
    import event_based_bos_amd as ebos

    parts = [_window(20_000, (), seed=33), _giant_window(30_000), _giant_window(100_000)]
    bounds = np.concatenate([[0], np.cumsum([len(p[2]) for p in parts])])
    r, c = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    t = np.concatenate([p[2] + 600_000 * k for k, p in enumerate(parts)])
    cols = tuple(torch.from_numpy(v).cuda() for v in (c.astype(np.int16), r.astype(np.int16), t.astype(np.int32), np.zeros(len(t), np.uint8)))
    ranges = [(int(bounds[k]), int(bounds[k + 1])) for k in range(3)]
    plans = ebos.EventPlan.build_raw_batch(*cols, ranges, SIZE, "first", True, tile=TILE, deferred=True)
    assert len(plans) == 3
    for k, ((a, b), plan) in enumerate(zip(ranges, plans)):
        got = _arrays(plan)
        assert k == 0 or np.diff(got[0]).max() == (30_000, 100_000)[k - 1]
        single = ebos.EventPlan.build_raw(*(v[a:b] for v in cols), SIZE, "first", True, tile=TILE, deferred=True, emit="compact")
        _assert_same(got, _arrays(single), f"window {k}")
        _assert_reference(got, _reference(_events_f64(r[a:b], c[a:b], t[a:b])), f"window {k}")


def test_deferred_build():
    """``deferred=True`` (no read-back of the build's facts) gives the same arrays."""
    r, c, t = _giant_window(30_000)
    build, ev64 = _source("raw32", r, c, t)
    got, now = _arrays(build(deferred=True)), _arrays(build(deferred=False))
    assert np.diff(got[0]).max() == 30_000
    _assert_same(got, now, "deferred")
    _assert_reference(got, _reference(ev64), "deferred")


def test_two_builds_solve_identically():
    """Three separately built plans of the 30 000-run window through the 2-DoF Adam loop on the blurred contrast (blur sigma 3, lr
    0.05, 100 iterations): the backward sweep sums a group's events in slot order, so equal slots are equal loss histories -- in the
    mode ``run`` picks by default (the resident launch, unless its rule refuses the crowded window: status -104) and with
    ``resident=False``."""
    from event_based_bos_amd.solver.fused_loop import Fused2dofLoop

    r, c, t = _giant_window(30_000)
    build, _ = _source("aos_f64", r, c, t)
    plans = [build() for _ in range(3)]
    for resident in (None, False):
        losses, modes = [], []
        for p in plans:
            loop = Fused2dofLoop(p, torch.zeros(2), 1.0, False, 0, "auto", lr=0.05, capacity=128, blur_sigma=3.0)
            losses.append(loop.run(100, resident=resident).cpu().numpy().copy())
            modes.append((loop.last_run_mode, loop.resident_status))
        print(f"resident={resident}: ran as {modes}")
        assert len(set(modes)) == 1, modes
        assert resident is None or modes[0][0] == "pipeline"
        assert np.isfinite(losses[0]).all() and np.ptp(losses[0]) > 0
        np.testing.assert_array_equal(losses[0], losses[1], err_msg=str(modes[0]))
        np.testing.assert_array_equal(losses[0], losses[2], err_msg=str(modes[0]))
