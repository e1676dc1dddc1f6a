"""The cases of tests/_bwd_loop_cases.py, pinned without a GPU, so that a failure of tests/test_gpu_bwd_loop_boundaries.py is never a
broken case: the tiles hold exactly the events and chunks the sets are named for, no pixel outside the hot-pixel case holds enough
events to take bits from the fixed-point unit (the per-tile allowance of the GPU test rests on 21 bits), the plain displacements stay
inside the smallest built halo, and in every spill case events of a work item of more than 32 chunks do leave their window -- from
chunks the queue hands out, not only from the pre-assigned ones."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bwd_loop_cases as B  # noqa: E402
from _bwd_loop_cases import GEOMETRIES, NONLEAN_SETS, SETS  # noqa: E402

ALL_WINDOWS = [(g[1], s) for g in GEOMETRIES for s in SETS]


@pytest.mark.parametrize("tile,name", ALL_WINDOWS, ids=[f"{t[0]}x{t[1]}-{s}" for t, s in ALL_WINDOWS])
def test_tiles_hold_the_events_and_chunks_of_their_set(tile, name):
    size, tile = B.geometry_of(tile)
    ev = B.window(tile, name)
    assert B.tile_counts(ev, size, tile) == SETS[name] and len(ev) == sum(SETS[name])
    assert tuple(B.chunks_of(n) for n in SETS[name]) == B.CHUNKS[name]
    assert tuple(-(-(-(-n // 4)) // 64) for n in SETS[name]) == B.CHUNKS[name]                 # ceil(ceil(n / 4) / 64), spelled out
    assert np.all(np.diff(ev[:, 2]) >= 0) and ev[0, 2] == 0.0 and ev[-1, 2] == 0.5              # sorted, covering the window
    assert np.all(ev[:, :2] == np.floor(ev[:, :2]))                                             # integer pixels: a lean plan
    # no source pixel takes a bit from the unit: below 64 events en <= 6, and bwd_fx_unit gives min(28 - en, 21) = 21 bits
    assert B.pixel_counts(ev, size).max() < 64
    # every plain displacement stays inside the smallest built halo
    disp = np.abs(B.warped(ev, B.flow(size)) - ev[:, :2])
    assert disp.max() <= B.FLOW_AMP < B.HALO_MIN
    for triple in B.TRIPLES:
        if triple[:2] == tile:
            assert not B.beyond_window(ev, B.flow(size), size, tile, triple[2]).any()


def test_sets_sit_on_the_seams_of_the_loop():
    assert max(B.CHUNKS["c"]) == B.PRE_ASSIGNED and min(B.CHUNKS["d"]) == B.PRE_ASSIGNED + 1      # the last without, the first with a live draw
    assert B.CHUNKS["d"] == (33, 34, 35, 36) and B.CHUNKS["e"] == (49, 65, 81, 97)
    assert SETS["d"][0] == 8192 + 1 and all(n % 256 == 1 for n in SETS["d"] + SETS["e"])         # last chunk: one group, one live event
    assert all(c % B.WAVES == 1 for c in B.CHUNKS["e"])                                          # the waves of a tile cannot share evenly
    assert [c // B.WAVES for c in B.CHUNKS["e"]] == [3, 4, 5, 6]                                 # 3 | 4 .. 6 | 7 chunks per wave: every place of the rotation
    assert SETS["b"][3] == 4 * 64 * 15 + 2 and B.CHUNKS["b"][3] == 16                            # a partial chunk on wave 15
    assert SETS["a"] == (0, 1, 3, 4)
    groups = [[-(-n // 4) for n in NONLEAN_SETS[s]] for s in "fg"]
    assert groups == [[1023, 1024, 1025, 2048], [2049, 1023, 1024, 1025]] and B.BLOCK == 1024
    assert B.TRIPLES[0] == B.MAIN and {t[:2] for t in B.TRIPLES} == {g[1] for g in GEOMETRIES}
    for name in "fg":
        for frac in (False, True):
            size, tile = GEOMETRIES[0]
            ev = B.window(tile, name, fractional=frac)
            assert B.tile_counts(ev, size, tile) == NONLEAN_SETS[name]
            assert bool(np.any(ev[:, :2] != np.floor(ev[:, :2]))) == frac
            assert np.abs(B.warped(ev, B.flow(size)) - ev[:, :2]).max() <= B.FLOW_AMP


def test_work_item_model_splits_every_set_but_the_smallest():
    """``ebos_plan_parts`` in Python, on 256 compute units: the GPU test runs splits = 0 on the sets it cuts a tile of and asserts the
    plan's part table against this."""
    parts = {s: B.adaptive_parts(SETS[s]) for s in SETS}
    assert parts == {"a": (1, 1, 1, 1), "b": (1, 1, 1, 5), "c": (1, 2, 2, 2), "d": (2, 2, 2, 2), "e": (1, 2, 2, 2)}
    assert all(sum(p) <= 8 for p in parts.values())
    # set e cut in two still gives work items past 32 chunks
    assert [B.chunks_of(-(-n // p)) for n, p in zip(SETS["e"], parts["e"])] == [49, 33, 41, 49]


@pytest.mark.parametrize("triple", [(45, 80, 32), (32, 32, 8)], ids=lambda t: "x".join(map(str, t)))
def test_row_of_40_px_spills_from_chunks_the_queue_hands_out(triple):
    tile, halo = triple[:2], triple[2]
    size, tile = B.geometry_of(tile)
    ev, fl = B.window(tile, "e"), B.row_flow(size, tile)
    out = B.beyond_window(ev, fl, size, tile, halo)
    k, chunk = B.tile_index(ev, size, tile), B.first_chunk(ev, size, tile)
    assert SETS["e"][3] == 24577 and B.chunks_of(24577) > B.PRE_ASSIGNED
    late = out & (k == 3) & (chunk >= B.PRE_ASSIGNED)
    print(f"{triple}: {int(out.sum())} events beyond the window, {int((out & (k == 3)).sum())} of tile 3, {int(late.sum())} in chunks >= 32")
    assert late.sum() > 0
    assert np.all(ev[out, 0] == B.spill_row(size, tile))                                        # only the row spills
    assert not B.beyond_window(ev, B.flow(size), size, tile, halo).any()


@pytest.mark.parametrize("name", ["d", "e"])
def test_field_of_30_px_reaches_the_spike_only_through_spilled_taps(name):
    size, tile = B.geometry_of((32, 32))
    ev, fl = B.window(tile, name), B.aimed_flow(size, tile)
    assert np.abs(fl).max() <= B.BIG_FLOW_AMP and (fl != B.big_flow(size)).sum() == 2 * 3 * 9
    spike = B.spike_pixel(tile)
    assert spike == (20, 20) and B.spike_upstream(size, tile)[spike] == B.SPIKE
    assert np.abs(np.delete(B.spike_upstream(size, tile).ravel(), spike[0] * size[1] + spike[1])).max() <= 1.0
    # outside the halo-8 window of tiles 1, 2 and 3 (its own tile, 0, stages it: an outlier, f64 from the start)
    assert spike[0] < tile[0] - B.HALO_MIN - 1 and spike[1] < tile[1] - B.HALO_MIN - 1
    out, hit = B.beyond_window(ev, fl, size, tile, B.HALO_MIN), B.touches(ev, fl, spike)
    k, chunk = B.tile_index(ev, size, tile), B.first_chunk(ev, size, tile)
    assert np.all(out[hit & (k != 0)])                                                          # only through spilled taps
    big = [t for t in range(1, 4) if B.chunks_of(SETS[name][t]) > B.PRE_ASSIGNED]
    assert big == [1, 2, 3]
    n_hit = {t: int((hit & (k == t)).sum()) for t in big}
    n_late = {t: int((out & (k == t) & (chunk >= B.PRE_ASSIGNED)).sum()) for t in big}
    late_hits = int((hit & (k == 3) & (chunk >= B.PRE_ASSIGNED)).sum())
    print(f"set {name}: events reaching the spike through the spill sweep {n_hit} ({late_hits} of tile 3 from chunks >= 32), "
          f"spilled events in chunks >= 32 {n_late}")
    assert n_hit[3] > 0 and all(v > 0 for v in n_late.values())
    if name == "e":   # (in set d the chunks past 32 are the tile's last three rows, 41 px from the spike: the field's 30 px do not reach)
        assert late_hits > 0


def test_before_plans_double_the_time_bound():
    """Reference time "before": dt in [1, 2] -- the displacements stay inside a halo of 32 (10 px), not of 8."""
    size, tile = GEOMETRIES[0]
    ev = B.window(tile, "e")
    disp = np.abs(B.warped(ev, B.flow(size), "before") - ev[:, :2])
    assert 2 * B.FLOW_AMP - 0.5 < disp.max() <= 2 * B.FLOW_AMP
    assert not B.beyond_window(ev, B.flow(size), size, tile, 32, "before").any()


def test_hot_pixel_case():
    size, tile = GEOMETRIES[0]
    ev = B.window(tile, "e", hot=B.HOT)
    assert B.tile_counts(ev, size, tile) == SETS["e"]
    counts = B.pixel_counts(ev, size)
    rs, cs = B.tile_slices(size, tile)[B.HOT[0]]
    assert counts[rs, cs].max() >= B.HOT[1] >= B.HOT_MIN and counts[rs, cs].sum() == 24577 > 8192
    cold = counts.copy()
    cold[rs, cs] = 0
    assert cold.max() < 64                                                                      # the other tiles stay fixed point


def test_forward_redo_and_batch_windows():
    size, tile = GEOMETRIES[0]
    ev = B.window(tile, "e", hot=B.HOT_WRAP)
    assert B.tile_counts(ev, size, tile) == SETS["e"]
    assert B.pixel_counts(ev, size).max() >= B.HOT_WRAP[1] and B.HOT_WRAP[1] * 2 ** 20 >= 2 ** 32     # the field wraps
    ws = B.batch_windows(tile)
    assert [B.tile_counts(w, size, tile) for w in ws] == [B.BATCH_OTHERS + (n,) for n in B.BATCH_TILE3]
    assert B.BATCH_TILE3 == (0, 8193, 1, 24577, 0) and all(len(w) > 0 for w in ws)


def test_run_time_window_cases():
    """halo="auto": the speculative window of the backward's set-up is 4 px and suffices where ceil(max |flow| x max |dt|) + 1 <= 4
    (halo_for): a field of 2.5 px; 20 px on a whole tile needs the real window, staged a round trip later -- both stay inside the
    largest built halo (no spill)."""
    size, tile = GEOMETRIES[0]
    ev = B.window(tile, "e")
    fl = B.reach_flow(size, tile)
    k = B.tile_index(ev, size, tile)
    disp = np.abs(B.warped(ev, fl) - ev[:, :2])
    assert disp[k == 3].max() > 19.0 and disp[k != 3].max() <= B.FLOW_AMP
    assert not B.beyond_window(ev, fl, size, tile, 32).any()
    small = B.flow(size, amp=B.SPEC_FLOW_AMP)
    assert np.ceil(np.abs(small).max()) + 1 <= 4 and np.abs(B.warped(ev, small) - ev[:, :2]).max() <= B.SPEC_FLOW_AMP


def test_yardstick_and_allowance():
    size, tile = GEOMETRIES[0]
    ev = B.window(tile, "a")
    g = B.ref_upstream_grad(("a", tile), ev, B.flow(size), B.upstream(size), size)
    counts = B.pixel_counts(ev, size)
    assert g.shape == (2,) + size and np.all(g[:, counts == 0] == 0.0)                          # a pixel's gradient depends on its own events only
    assert B.ref_upstream_grad(("a", tile), ev, B.flow(size), B.upstream(size), size) is g      # computed once
    assert np.abs(B.upstream(size)).max() <= 1.0
    one = np.zeros(size, dtype=np.int64)
    one[3, 3] = 1
    assert B.allowance(one, 1.0) == 0.5 * 2.0 ** -19 * np.sqrt(2.0)
    assert B.allowance(counts, 1.0) == 0.5 * 2.0 ** -19 * np.sqrt(2.0 * (counts.astype(float) ** 2).sum())
