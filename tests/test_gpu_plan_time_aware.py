"""GPU tests of the batched time-aware plan build from raw sensor columns (``ebos_plan_time_aware_raw_batch``,
``TimeAwarePlanStack.from_raw`` / ``EventPlan.build_raw_batch_time_aware``).

Yardstick: the route the build replaces, window by window -- ``window_ingest_raw_batch`` on the same columns supplies
``PreparedWindows.events(b)``, ``EventPlan.build(events, image, direction, True, tile=tile, emit="full", time_bin=T)`` plans them and
``EventPlan.stack_time_aware`` stacks them.  The two builds agree bit for bit once every source pixel's run is ordered by the events'
source index (the order inside a run is unspecified in both).  Shapes and ranges: tests/_plan_time_aware_cases.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _plan_time_aware_cases as K  # noqa: E402
import _warp_voxel_ref as R  # noqa: E402

from oracle import ebos_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


@pytest.fixture(scope="module")
def lib(ebos):
    from event_based_bos_amd import _hip

    return _hip.require_gpu()


def build_new(ebos, geometry, t64, rect, direction, T, ranges=None):
    (H, W), tile = K.GEOMETRIES[geometry]
    cols = K.device_columns(geometry, t64)
    roi, remove = K.RECTS[rect]
    ranges = K.ranges_of(len(cols[2])) if ranges is None else ranges
    return ebos.TimeAwarePlanStack.from_raw(cols, ranges, (H, W), direction, tile, T, roi=roi, remove=remove,
                                            ticks_per_second=K.TICKS_PER_SECOND)


def build_yardstick(ebos, geometry, t64, rect, direction, T):
    """[(plan, index of every event of events(b) inside its range)] for the non-empty ranges, through the existing route."""
    from event_based_bos_amd.evaluation import window_ingest_raw_batch

    (H, W), tile = K.GEOMETRIES[geometry]
    cols = K.device_columns(geometry, t64)
    roi, remove = K.RECTS[rect]
    ranges = K.ranges_of(len(cols[2]))
    prepared = window_ingest_raw_batch(cols, ranges, (H, W), roi, remove, K.TICKS_PER_SECOND)
    col, row = (c.cpu().numpy() for c in cols[:2])
    out = []
    for b, (lo, hi) in enumerate(ranges):
        if hi == lo:
            out.append(None)
            continue
        plan = ebos.EventPlan.build(prepared.events(b), (H, W), direction, True, tile=tile, emit="full", time_bin=T)
        out.append((plan, np.nonzero(K.keep_mask(col[lo:hi], row[lo:hi], roi, remove))[0]))
    return out


# ---------------------------------------------------------------------------------------------- 1. against the existing route
@pytest.mark.parametrize("direction", ["first", "middle"])
@pytest.mark.parametrize("rect", list(K.RECTS))
@pytest.mark.parametrize("t64", [False, True])
@pytest.mark.parametrize("T", [1, 5, 255])
@pytest.mark.parametrize("geometry", list(K.GEOMETRIES))
def test_stack_from_raw_equals_the_window_by_window_build(ebos, geometry, T, t64, rect, direction):
    (H, W), tile = K.GEOMETRIES[geometry]
    stack = build_new(ebos, geometry, t64, rect, direction, T)
    yard = build_yardstick(ebos, geometry, t64, rect, direction, T)
    n_keys = -(-H // tile[0]) * -(-W // tile[1]) * tile[0] * tile[1]
    assert len(stack) == 6 and stack.time_bin == T and stack.image_size == (H, W) and stack.tile == tile
    assert stack.key_offsets.shape == (6, n_keys + 1) and stack.key_offsets.dtype == torch.int32
    assert stack.n == sum(stack.ns) and stack.x.shape[0] == stack.n
    # the empty range: a constant row, no events
    empty = stack.plans[0]
    assert stack.ns[0] == 0 and empty.n == 0 and empty.n_dropped == 0 and int(empty.key_offsets.abs().max()) == 0
    assert bool((stack.key_offsets[0] == 0).all())
    kept = []
    for b in range(1, 6):
        plan, src = yard[b]
        new = stack.plans[b]
        assert (new.n, new.n_dropped, new.n_input) == (plan.n, plan.n_dropped, plan.n_input), b
        assert new.n == stack.ns[b] and new.time_bin == T and new.dt_bound == plan.dt_bound and new.part_table is None
        assert torch.equal(new.key_offsets, plan.key_offsets), b
        assert K.same_plan(K.canonical(new), K.canonical(plan, src)), b
        kept.append(plan)
    assert stack.ns[1] == 1 and stack.ns[2] == 2                     # (the degenerate windows keep their events: NaN dt compared as bits)
    assert bool(torch.isnan(stack.plans[2].dt).all()) and int(stack.plans[2].bins.max()) == 0
    if rect in ("none", "roi"):                                      # the stuck pixel's run, over every bin
        ko = stack.plans[5].key_offsets.cpu().numpy()
        assert np.diff(ko).max() >= K.HOT_EXTRA
    assert any(p.n_dropped > 0 for p in kept) == (rect in ("none", "remove"))   # (the CROP rectangle lies inside the image)
    want = ebos.EventPlan.stack_time_aware(kept)
    assert torch.equal(stack.key_offsets[1:], want.key_offsets)
    assert stack.n == want.n


# ---------------------------------------------------------------------------------------------- 2. output buffers
def test_outputs_are_written_inside_their_bounds_only(ebos, lib):
    from event_based_bos_amd._hip import stream_ptr

    geometry, T = "37x70", 5
    (H, W), tile = K.GEOMETRIES[geometry]
    cols = K.device_columns(geometry, False)
    ranges = K.ranges_of(len(cols[2]))
    B, total = len(ranges), sum(e - b for b, e in ranges)
    n_keys = -(-H // tile[0]) * -(-W // tile[1]) * tile[0] * tile[1]
    guard = 4096

    def guarded(n, dtype):
        """(the bytes of the whole buffer, every one 0xFF; the view of n elements with ``guard`` elements in front and behind)"""
        raw = torch.full(((guard + n + guard) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=K.dev())
        return raw, raw.view(dtype)[guard:guard + n]

    bufs = {k: guarded(total, dt) for k, dt in (("x", torch.float32), ("y", torch.float32), ("dt", torch.float32), ("bins", torch.uint8),
                                                ("perm", torch.int32))}
    bufs["local"] = guarded(B * (n_keys + 1), torch.int32)
    bufs["stacked"] = guarded(B * (n_keys + 1), torch.int32)
    bufs["counts"] = guarded(B * 2, torch.int32)
    bufs["tminmax"] = guarded(B * 2, torch.float64)
    c_ranges = (ctypes.c_int64 * (2 * B))(*[v for r in ranges for v in r])
    nbytes = int(lib.ebos_plan_time_aware_batch_scratch_bytes(c_ranges, B, H, W, *tile))
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=K.dev())
    v = {k: b[1] for k, b in bufs.items()}
    rc = lib.ebos_plan_time_aware_raw_batch(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), 0, K.TICKS_PER_SECOND, len(cols[2]),
                                            c_ranges, B, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 1, T, H, W, tile[0], tile[1],
                                            v["x"].data_ptr(), v["y"].data_ptr(), v["dt"].data_ptr(), v["bins"].data_ptr(),
                                            v["perm"].data_ptr(), total, v["local"].data_ptr(), v["stacked"].data_ptr(), n_keys + 1,
                                            v["counts"].data_ptr(), v["tminmax"].data_ptr(), scratch.data_ptr(), nbytes, stream_ptr())
    assert rc == 0, lib.ebos_last_error()
    torch.cuda.synchronize()
    for k, (raw, view) in bufs.items():
        g = guard * view.element_size()
        assert bool((raw[:g] == 0xFF).all()) and bool((raw[-g:] == 0xFF).all()), k
    counts = v["counts"].view(B, 2).cpu().numpy()
    kept = int(counts[:, 0].sum())
    assert 0 < kept < total and (counts >= 0).all()
    for k in ("x", "y", "dt", "perm"):
        as_int = v[k].view(torch.int32)
        assert bool((as_int[:kept] != -1).all()), k                 # every element of [0, sum n_b) was written ...
        assert bool((as_int[kept:] == -1).all()), k                 # ... and nothing behind it
    assert bool((v["bins"][:kept] < T).all()) and bool((v["bins"][kept:] == 0xFF).all())
    assert bool((v["local"] != -1).all()) and bool((v["stacked"] != -1).all())
    tmm = v["tminmax"].view(B, 2).cpu().numpy()
    ticks = K.raw_columns(geometry)[2]
    assert np.array_equal(tmm[0], [0.0, 0.0])
    for b, (lo, hi) in enumerate(ranges[1:], start=1):
        assert np.array_equal(tmm[b], [ticks[lo:hi].min() / K.TICKS_PER_SECOND, ticks[lo:hi].max() / K.TICKS_PER_SECOND]), b
    # the same call through the host layer gives the same counts
    stack = build_new(ebos, geometry, False, "none", "first", T)
    assert stack.ns == counts[:, 0].tolist()


# ---------------------------------------------------------------------------------------------- 3. independence
def test_windows_do_not_depend_on_their_place_in_the_batch(ebos):
    geometry, T = "37x70", 5
    n = len(K.raw_columns(geometry)[0])
    ranges = K.ranges_of(n)
    order = [4, 0, 5, 2, 1, 3]
    a = build_new(ebos, geometry, True, "both", "middle", T)
    b = build_new(ebos, geometry, True, "both", "middle", T, ranges=[ranges[k] for k in order])
    assert b.ns == [a.ns[k] for k in order]
    bases = np.concatenate([[0], np.cumsum(b.ns)])
    for at, k in enumerate(order):
        assert torch.equal(b.plans[at].key_offsets, a.plans[k].key_offsets), k
        assert K.same_plan(K.canonical(b.plans[at]), K.canonical(a.plans[k])), k
        assert torch.equal(b.key_offsets[at], a.plans[k].key_offsets + int(bases[at])), k
    # a batch of one gives the window too
    one = build_new(ebos, geometry, True, "both", "middle", T, ranges=[ranges[3]])
    assert K.same_plan(K.canonical(one.plans[0]), K.canonical(a.plans[3])) and torch.equal(one.key_offsets[0], a.plans[3].key_offsets)


# ---------------------------------------------------------------------------------------------- 4. operators on the views
@pytest.mark.parametrize("geometry", list(K.GEOMETRIES))
def test_operators_on_the_views(ebos, geometry):
    T = 5
    (H, W), tile = K.GEOMETRIES[geometry]
    stack = build_new(ebos, geometry, False, "none", "first", T)
    yard = build_yardstick(ebos, geometry, False, "none", "first", T)
    assert stack.plans[3].resolve_splits(None) == 1
    vx = np.random.RandomState(5).uniform(-4.0, 4.0, (T, 2, H, W))
    voxel = torch.from_numpy(vx).to(K.dev(), torch.float32)
    col, row, ticks, pol = K.raw_columns(geometry)
    for b in (3, 5):                                                 # the 20 000-event range and the whole store (with the stuck pixel)
        new, (plan, _) = stack.plans[b], yard[b]
        for patch in ((12, 14), (8, 8)):
            assert torch.equal(new.patch_event_counts(patch, patch), plan.patch_event_counts(patch, patch)), (b, patch)
        assert torch.equal(new.pixel_event_counts(), plan.pixel_event_counts()), b
        got, old = new.iwe_voxel(voxel), plan.iwe_voxel(voxel)
        lo, hi = K.ranges_of(len(col))[b]
        ev = np.stack([row[lo:hi], col[lo:hi], ticks[lo:hi] / K.TICKS_PER_SECOND, pol[lo:hi]], axis=1).astype(np.float64)
        inside = (ev[:, 0] >= 0) & (ev[:, 0] < H) & (ev[:, 1] >= 0) & (ev[:, 1] < W)
        assert inside[0] and inside[-1] or b == 5                     # (range 3 keeps its first and last event: the same time range)
        if b == 5:                                                    # the time range is the whole range's: pin it with two events of no weight
            ev = np.concatenate([ev, [[K.INSIDE[0], K.INSIDE[1], ev[:, 2].min(), 0.0], [K.INSIDE[0], K.INSIDE[1], ev[:, 2].max(), 0.0]]])
            inside = np.concatenate([inside, [True, True]])
            weight = np.concatenate([np.ones(hi - lo), [0.0, 0.0]])[inside]
        else:
            weight = np.ones(int(inside.sum()))
        order = np.argsort(ev[inside][:, 2], kind="stable")
        want = R.iwe_voxel(torch.from_numpy(ev[inside][order]), torch.from_numpy(vx), "first", True, (0, 0),
                           weight=torch.from_numpy(weight[order])).numpy()
        r_new, r_old = O.rel_l2(got.cpu().numpy().astype(np.float64), want), O.rel_l2(old.cpu().numpy().astype(np.float64), want)
        print(f"{geometry} window {b}: IWE relative L2 against float64: views {r_new:.3e}, window-by-window build {r_old:.3e}")
        assert r_new < 1e-4 and r_old < 1e-4, (b, r_new, r_old)


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_the_entry_point_refuses_bad_arguments(lib):
    """Everything is validated before the first launch: EBOS_ERR_INVALID_ARG (-1), nothing enqueued -- the outputs keep their fill."""
    from event_based_bos_amd import _hip
    from event_based_bos_amd._hip import stream_ptr

    H, W, th, tw, T = 37, 70, 32, 32, 5
    n = 1000
    col = torch.zeros(n, dtype=torch.int16, device=K.dev())
    row = torch.zeros(n, dtype=torch.int16, device=K.dev())
    t = torch.arange(n, dtype=torch.int32, device=K.dev())
    n_keys = 2 * 3 * th * tw
    cap = 1200                                                        # the two good ranges hold 600 events each
    out = {k: torch.full(((cap + 8) * (1 if k == "bins" else 4),), 0xFF, dtype=torch.uint8, device=K.dev()) for k in ("x", "y", "dt", "bins", "perm")}
    keys = torch.full((2, 2, n_keys + 1), -1, dtype=torch.int32, device=K.dev())
    counts = torch.full((2, 2), -1, dtype=torch.int32, device=K.dev())
    tmm = torch.full((2, 2), -1.0, dtype=torch.float64, device=K.dev())
    good_ranges = [0, 600, 400, 1000]
    nbytes = int(lib.ebos_plan_time_aware_batch_scratch_bytes((ctypes.c_int64 * 4)(*good_ranges), 2, H, W, th, tw))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=K.dev())

    def call(ranges=good_ranges, B=2, T=T, roi=(0, 0, 0, 0, 0), rm=(0, 0, 0, 0, 0), n_total=n, capacity=cap, colp=None, xp=None, ref_mode=0,
             scratch_bytes=nbytes, key_stride=n_keys + 1, rangesp=True):
        c_ranges = (ctypes.c_int64 * len(ranges))(*ranges) if rangesp else None
        return lib.ebos_plan_time_aware_raw_batch(col.data_ptr() if colp is None else colp, row.data_ptr(), t.data_ptr(), 0, 1e6, n_total,
                                                  c_ranges, B, *roi, *rm, ref_mode, 0.0, 1, T, H, W, th, tw,
                                                  out["x"].data_ptr() if xp is None else xp, out["y"].data_ptr(), out["dt"].data_ptr(),
                                                  out["bins"].data_ptr(), out["perm"].data_ptr(), capacity, keys[0].data_ptr(),
                                                  keys[1].data_ptr(), key_stride, counts.data_ptr(), tmm.data_ptr(), scratch.data_ptr(),
                                                  scratch_bytes, stream_ptr())

    bad = {
        "B = 0": dict(B=0),
        "B too large": dict(B=_hip.CMAX_VOXEL_MAX_BATCH + 1, ranges=[0, 1] * (_hip.CMAX_VOXEL_MAX_BATCH + 1)),
        "T = 0": dict(T=0),
        "T = 256": dict(T=256),
        "NULL ranges": dict(rangesp=False),
        "NULL column": dict(colp=0),
        "NULL output": dict(xp=0),
        "range past the columns": dict(ranges=[0, 600, 400, 1001]),
        "range reversed": dict(ranges=[600, 0, 400, 1000]),
        "negative begin": dict(ranges=[-1, 600, 400, 1000]),
        "capacity": dict(capacity=1199),
        "roi order": dict(roi=(1, 10, 5, 0, 70)),
        "removal order": dict(rm=(1, 0, 5, 70, 0)),
        "ref mode": dict(ref_mode=3),
        "key stride": dict(key_stride=n_keys),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert lib.ebos_last_error(), what
    assert call(scratch_bytes=nbytes - 1) != 0                        # (EBOS_ERR_SCRATCH, the code of every entry point with scratch)
    total = (ctypes.c_int64 * 4)(0, 2 ** 31 - 1, 0, 1)
    assert int(lib.ebos_plan_time_aware_batch_scratch_bytes(total, 2, H, W, th, tw)) == 0      # more than INT32_MAX events in total
    torch.cuda.synchronize()
    assert all(bool((v == 0xFF).all()) for v in out.values()) and bool((keys == -1).all()) and bool((counts == -1).all())
    assert bool((tmm == -1.0).all())
    assert call() == 0                                                # the arguments the refusals vary are good ones
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [[600, 0], [600, 0]]
