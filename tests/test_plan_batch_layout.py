"""Host side of the batched plan build (``EventPlan.build_raw_batch``): where every window's arrays lie in the batch's buffers
(``plan_batch_layout``, pure Python) and how much scratch ``ebos_plan_lean_batch`` asks for (a host-only query).  No GPU needed."""
import ctypes as C

import pytest

from event_based_bos_amd import _hip
from event_based_bos_amd.event_plan import PLAN_BATCH_ALIGN, plan_batch_layout

GEOMS = [((64, 96), (32, 32)), ((100, 150), (32, 64)), ((90, 160), (45, 80)), ((720, 1280), (45, 80))]


def _tiles(size, tile):
    return -(-size[0] // tile[0]) * -(-size[1] // tile[1])


@pytest.mark.parametrize("size,tile", GEOMS)
def test_layout_offsets_are_disjoint_aligned_and_sized_like_the_single_build(size, tile):
    lengths = [700, 0, 1, 9, 6001, 0, 123_457]
    lay = plan_batch_layout(lengths, size, tile)
    n_tiles = _tiles(size, tile)
    assert lay.n_tiles == n_tiles and lay.n_keys == n_tiles * tile[0] * tile[1]
    # every window holds what EventPlan.build_raw allocates for it: n + 3 n_tiles + 8 slots, which covers what ebos_plan_lean asks for
    assert list(lay.capacities) == [n + 3 * n_tiles + 8 for n in lengths]
    assert len(lay.slot_offsets) == len(lengths) + 1 and lay.slot_offsets[0] == 0
    for w, n in enumerate(lengths):
        lo, hi = lay.slot_offsets[w], lay.slot_offsets[w + 1]
        assert lo % PLAN_BATCH_ALIGN == 0 and lo % 8 == 0          # 16-byte vectors of u16 pixels and f32 dt
        assert lo + lay.capacities[w] <= hi                        # disjoint: a window ends before the next begins
        assert hi - lo < lay.capacities[w] + PLAN_BATCH_ALIGN      # ... and nothing but the alignment is added
    # the per-window tables: rows of a [B, stride] array, each row long enough and aligned
    for stride, need in ((lay.key_stride, lay.n_keys + 1), (lay.grp_stride, n_tiles + 1), (lay.part_stride, 5 * n_tiles + 1)):
        assert need <= stride < need + PLAN_BATCH_ALIGN and stride % PLAN_BATCH_ALIGN == 0


def test_layout_of_one_window_is_the_single_window_layout():
    size, tile, n = (260, 346), (32, 32), 50_000
    lay = plan_batch_layout([n], size, tile)
    n_tiles = _tiles(size, tile)
    assert lay.slot_offsets[0] == 0 and lay.capacities == (n + 3 * n_tiles + 8,)
    assert lay.slot_offsets[1] >= lay.capacities[0]
    assert lay.n_keys + 1 <= lay.key_stride and n_tiles + 1 <= lay.grp_stride and 5 * n_tiles + 1 <= lay.part_stride


def test_layout_handles_empty_windows_and_refuses_nonsense():
    lay = plan_batch_layout([0, 0, 0], (64, 96), (32, 32))
    assert lay.capacities == (26, 26, 26) and lay.slot_offsets == (0, 64, 128, 192)    # 3 x 6 tiles + 8 slots each, kept apart
    assert plan_batch_layout([], (64, 96), (32, 32)).slot_offsets == (0,)
    with pytest.raises(ValueError):
        plan_batch_layout([5, -1], (64, 96), (32, 32))
    with pytest.raises(ValueError):
        plan_batch_layout([5], (64, 96), (0, 32))


def _ranges(lengths, start=0):
    flat, at = [], start
    for n in lengths:
        flat += [at, at + n]
        at += n
    return (C.c_int64 * len(flat))(*flat)


def test_batch_scratch_is_host_only_monotonic_and_covers_the_single_sizes():
    """``ebos_plan_lean_batch_scratch_bytes`` (no GPU touched): sized per window by the rule of ``ebos_plan_lean_scratch_bytes``, so it
    never shrinks when any window grows, is at least the sum of the single-window sizes, ignores where the ranges lie, and is zero
    for a bad geometry."""
    lib = _hip.load_library()
    one, many = lib.ebos_plan_lean_scratch_bytes, lib.ebos_plan_lean_batch_scratch_bytes
    H, W, th, tw = 720, 1280, 45, 80
    sizes = (0, 1, 7, 1000, 100_000, 2_000_000, 10_000_000)
    base = [1000, 0, 50_000]
    prev = [0, 0, 0]
    for n in sizes:
        for k in range(3):   # grow window k, the others fixed
            lengths = list(base)
            lengths[k] = n
            b = int(many(_ranges(lengths), 3, H, W, th, tw))
            assert b >= sum(int(one(m, H, W, th, tw)) for m in lengths), (lengths, b)
            assert b >= 10 * sum(lengths) and b >= prev[k], (lengths, b, prev[k])
            prev[k] = b
    assert int(many(_ranges([5000]), 1, H, W, th, tw)) == int(one(5000, H, W, th, tw))
    assert int(many(_ranges(base), 3, H, W, th, tw)) == int(many(_ranges(base, start=12345), 3, H, W, th, tw))
    overlap = (C.c_int64 * 4)(0, 4000, 2000, 6000)
    assert int(many(overlap, 2, H, W, th, tw)) == 2 * int(one(4000, H, W, th, tw))
    assert int(many(None, 3, H, W, th, tw)) == 0 and int(many(_ranges(base), 0, H, W, th, tw)) == 0
    assert int(many(_ranges(base), 3, 0, W, th, tw)) == 0 and int(many(_ranges(base), 3, H, W, th, 0)) == 0
    backwards = (C.c_int64 * 2)(10, 5)
    assert int(many(backwards, 1, H, W, th, tw)) == 0
