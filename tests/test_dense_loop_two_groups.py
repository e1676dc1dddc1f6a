"""The dense-field accumulate loop with two groups per trip (accumulate_compact_fx, TWO): chunk boundaries.

The loop of the single-window kernel that `launch_slab_fwd` picks for a compact unit-weight plan, dense flow and a built halo
handles two chunks of a wave per trip and draws its chunk indices one step ahead.  It can go wrong where chunks begin and end,
not at scale: a chunk is 64 groups = 256 events, a workgroup has 16 waves, chunks 0 .. 31 are pre-assigned, everything beyond
comes from the queue.  The cases below put chosen numbers of events into the four tiles of a 2 x 2-tile image (one work item per
tile: splits=1) and compare

  * with the run-time-window route (halo="auto"): another instantiation, the one-group loop, and both accumulate integers --
    images and variances bit for bit;
  * with the f64 oracle, at the tolerance of the existing dense-slab tests (rel-L2 < 1e-5);
  * a second call through the same workspace, bit for bit (a queue counter left in a wrong state would show here).
"""
import numpy as np
import pytest
import torch

from oracle import ebos_oracle as O

pytestmark = pytest.mark.gpu

SETS = {
    "a": (0, 1, 3, 4),
    "b": (255, 256, 257, 4 * 64 * 15 + 2),
    "c": (4096, 4100, 8191, 8192),          # exactly and just past 16 and 32 chunks
    "d": (8193, 8451, 12545, 12800),        # 33, 34, 49 and 50 chunks: odd and even numbers of chunks per wave beyond the pre-assigned
}
GEOMETRIES = [((90, 160), (45, 80)), ((128, 128), (64, 64)), ((64, 64), (32, 32))]
CASES = [(GEOMETRIES[0], s) for s in "abcd"] + [(g, "d") for g in GEOMETRIES[1:]]


def _events(size, tile, counts, seed, hot=None):
    """[n, 4] float64 events (row, column, t, p), times sorted in [0, 0.5): counts[k] events in tile k of the 2 x 2 tiles, uniform
    over the tile's pixels; hot = (k, m): m of tile k's events sit on ONE pixel."""
    (h, w), (th, tw) = size, tile
    assert (h, w) == (2 * th, 2 * tw)
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    for k, n in enumerate(counts):
        r0, c0 = (k // 2) * th, (k % 2) * tw
        r, c = rs.randint(0, th, n) + r0, rs.randint(0, tw, n) + c0
        if hot is not None and hot[0] == k:
            r[: hot[1]], c[: hot[1]] = r0 + th // 2, c0 + tw // 3
        rows.append(r), cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = rs.permutation(rows.size)
    t = np.sort(rs.uniform(0.0, 0.5, rows.size))
    return np.stack([rows[order], cols[order], t, rs.randint(0, 2, rows.size)], axis=1).astype(np.float64)


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.asarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _both_routes(ebos, ev, size, tile, fl):
    """IWE and variance through the built 32 px halo (twice) and through run-time windows, one work item per tile."""
    plan = ebos.EventPlan.build(_gpu(ev), size, "first", True, tile=tile, emit="compact")
    assert plan.compact and plan.n == ev.shape[0]
    flow = _gpu(fl, torch.float32)
    built = plan.iwe_dense(flow, halo=32, splits=1)
    again = plan.iwe_dense(flow, halo=32, splits=1)
    auto = plan.iwe_dense(flow, halo="auto", splits=1)
    v_built = plan.contrast_dense(flow, halo=32, splits=1).item()
    v_auto = plan.contrast_dense(flow, halo="auto", splits=1).item()
    return built, again, auto, v_built, v_auto


def _tile_counts(ev, size, tile):
    (h, w), (th, tw) = size, tile
    k = (ev[:, 0].astype(np.int64) // th) * 2 + ev[:, 1].astype(np.int64) // tw
    return tuple(np.bincount(k, minlength=4))


@pytest.mark.parametrize("geometry,name", CASES, ids=[f"{g[1][0]}x{g[1][1]}-{s}" for g, s in CASES])
def test_chunk_boundaries_match_run_time_windows_and_oracle(ebos, geometry, name):
    size, tile = geometry
    ev = _events(size, tile, SETS[name], seed=11 + ord(name))
    assert _tile_counts(ev, size, tile) == SETS[name]
    fl = np.random.RandomState(5).uniform(-30.0, 30.0, (2,) + size)
    built, again, auto, v_built, v_auto = _both_routes(ebos, ev, size, tile, fl)
    want = O.iwe_dense(torch.from_numpy(ev), torch.from_numpy(fl), size).numpy()
    err = O.rel_l2(built.cpu().numpy(), want)
    print(f"[{tile} set {name}: {SETS[name]}] built == auto {torch.equal(built, auto)}, variance {v_built!r} / {v_auto!r}, "
          f"repeat {torch.equal(built, again)}, oracle rel-L2 {err:.2e}")
    assert torch.equal(built, auto)
    assert v_built == v_auto
    assert torch.equal(built, again)
    assert err < 1e-5


@pytest.fixture(scope="module")
def set_c():
    size, tile = GEOMETRIES[0]
    return size, tile, _events(size, tile, SETS["c"], seed=23), np.random.RandomState(6).uniform(-30.0, 30.0, (2,) + size)


def test_nan_flow_masks_the_pixels_events(ebos, set_c):
    """A NaN flow value on a pixel that holds events: those events leave the image (the fixed-point sums disagree, the slice is
    redone exactly, and there the events are masked), on both routes alike."""
    size, tile, ev, fl = set_c
    r, c = int(ev[7, 0]), int(ev[7, 1])
    on_pixel = (ev[:, 0] == r) & (ev[:, 1] == c)
    assert on_pixel.sum() >= 1
    fl = fl.copy()
    fl[0, r, c] = np.nan
    built, again, auto, v_built, v_auto = _both_routes(ebos, ev, size, tile, fl)
    clean = fl.copy()
    clean[0, r, c] = 0.0
    want = O.iwe_dense(torch.from_numpy(ev[~on_pixel]), torch.from_numpy(clean), size).numpy()
    err = O.rel_l2(built.cpu().numpy(), want)
    print(f"[NaN flow at ({r}, {c}), {int(on_pixel.sum())} events] built == auto {torch.equal(built, auto)}, variance {v_built!r} / {v_auto!r}, "
          f"oracle (events removed) rel-L2 {err:.2e}")
    assert torch.isfinite(built).all()
    assert torch.equal(built, auto) and v_built == v_auto
    assert torch.equal(built, again)
    assert err < 1e-5


def test_flow_beyond_the_halo_spills(ebos, set_c):
    """40 px of flow on one pixel row: taps beyond the 32 px window go to the spill image through float atomics -- compared with the
    oracle (and the other route) at the spill tolerances of the existing tests, not bit for bit."""
    size, tile, ev, fl = set_c
    fl = fl.copy()
    fl[0, 50, :] = 40.0
    fl[1, 50, :] = -40.0
    built, again, auto, v_built, v_auto = _both_routes(ebos, ev, size, tile, fl)
    want = O.iwe_dense(torch.from_numpy(ev), torch.from_numpy(fl), size).numpy()
    err, err_auto = O.rel_l2(built.cpu().numpy(), want), O.rel_l2(built.cpu().numpy(), auto.cpu().numpy())
    print(f"[40 px row] oracle rel-L2 {err:.2e}, against run-time windows {err_auto:.2e}, repeat {O.rel_l2(again.cpu().numpy(), built.cpu().numpy()):.2e}")
    assert err < 1e-5
    assert err_auto < 1e-6
    assert O.rel_l2(again.cpu().numpy(), built.cpu().numpy()) < 1e-6


def test_hot_pixel_wraps_the_field_and_is_redone_exactly(ebos):
    """5 000 events on one pixel under zero flow: 5 000 x 2^20 does not fit the 32-bit field, the checksum notices and the exact f64
    loop redoes the slice (it draws its chunks afresh from the same queue)."""
    size, tile = GEOMETRIES[0]
    ev = _events(size, tile, SETS["c"], seed=29, hot=(3, 5000))
    fl = np.zeros((2,) + size)
    built, again, auto, v_built, v_auto = _both_routes(ebos, ev, size, tile, fl)
    counts = np.bincount(ev[:, 0].astype(np.int64) * size[1] + ev[:, 1].astype(np.int64), minlength=size[0] * size[1]).reshape(size)
    print(f"[hot pixel] max {built.max().item()}, built == auto {torch.equal(built, auto)}, variance {v_built!r} / {v_auto!r}")
    assert counts.max() >= 5000
    assert np.array_equal(built.cpu().numpy(), counts.astype(np.float32))  # zero flow: the event histogram, exact
    assert torch.equal(built, auto) and v_built == v_auto
    assert torch.equal(built, again)
