"""``EventPlan.build_raw_batch`` / ``RawEventStore.plans`` / ``WindowPipeline(batch_ingest=True)``: the plans of several windows of one
recording built by one set of launches.  The definition throughout is the single build -- ``EventPlan.build_raw`` on the window's slice
of the columns, ``emit="compact"`` -- and, the builds being canonical (two builds of one window are identical arrays), the bar is
equality of bits: key_offsets, grp_offsets, the defined slots of cpix / cdt, counts and part_table."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GEOMS = {"64x96/32x32": ((64, 96), (32, 32)), "100x150/32x64": ((100, 150), (32, 64)), "90x160/45x80": ((90, 160), (45, 80))}
# segments of the synthetic recording, in the order they lie in the columns
SEGMENTS = (("A", 6000), ("B", 700), ("C", 9), ("D", 1), ("TILE", 500), ("HOT", 3200), ("OOB", 300))


def _recording(size, tile, t_dtype, seed=0):
    """Raw columns (numpy) and {segment: (begin, end)}.  TILE: every event in tile 0.  HOT: 3000 events on one pixel -- a run longer than
    one 16-lane sorting network, than the 1024 events ranked in place (kLeanCanon, plan_lean.hip) and than a chunk of the staging pass
    (a 3200-event window is cut into chunks of ~800) -- among 200 others.  OOB: five events outside the image."""
    H, W = size
    rs = np.random.RandomState(seed)
    cols, rows, at, seg = [], [], 0, {}
    for name, n in SEGMENTS:
        r, c = rs.randint(0, H, n), rs.randint(0, W, n)
        if name == "TILE":
            r, c = rs.randint(0, min(tile[0], H), n), rs.randint(0, min(tile[1], W), n)
        elif name == "HOT":
            hot = rs.permutation(n)[:3000]
            r[hot], c[hot] = H // 2 + 1, W // 2 + 3
        elif name == "OOB":
            r[[3, 70]], c[[150, 299]] = (-1, H), (W, W + 7)
            r[200], c[200] = H + 2, -4
        rows.append(r); cols.append(c)
        seg[name] = (at, at + n)
        at += n
    # ticks with repeats (equal dt inside a pixel), starting beyond 2^31 for the 64-bit recording
    t = np.cumsum(rs.randint(0, 3, at)) + (5_000_000_000 if t_dtype == np.int64 else 1_000_000)
    return (np.concatenate(cols).astype(np.int16), np.concatenate(rows).astype(np.int16), t.astype(t_dtype),
            rs.randint(0, 2, at).astype(np.uint8)), seg


def _batches(seg):
    A, B, Cs, D, T, HOT, OOB = (seg[k] for k in ("A", "B", "C", "D", "TILE", "HOT", "OOB"))
    empty = (B[1], B[1])
    return {
        "one": [A],
        "three": [B, empty, HOT],                                        # ~700, 0, 3200 (the hot pixel)
        "five": [Cs, A, D, empty, B],                                    # 9, ~6000, 1, 0, ~700
        "overlap": [(A[0], A[0] + 4000), (A[0] + 2000, B[1]), (A[0] + 3990, A[0] + 4010)],
        "unordered": [OOB, T, (A[0] + 100, A[0] + 900), Cs],             # descending begins; one tile; events outside the image
    }


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same_plan(got, ref, what):
    assert (got.image_size, got.tile, got.n, got.n_input, got.n_dropped, got.dt_bound) == \
           (ref.image_size, ref.tile, ref.n, ref.n_input, ref.n_dropped, ref.dt_bound), what
    assert got.lean and got.compact and ref.lean and ref.compact, what
    assert torch.equal(got.key_offsets, ref.key_offsets), what
    assert torch.equal(got.grp_offsets, ref.grp_offsets), what
    used = int(ref.grp_offsets[-1]) * 4
    assert got.cpix.numel() == ref.cpix.numel() and got.cdt.numel() == ref.cdt.numel(), what
    assert torch.equal(got.cpix[:used], ref.cpix[:used]), what
    assert torch.equal(_bits(got.cdt[:used]), _bits(ref.cdt[:used])), what     # (bits: the padding slots hold NaN)
    assert torch.equal(got.__dict__["_counts"], ref.__dict__["_counts"]), what
    assert torch.equal(got.part_table, ref.part_table), what
    assert got.__dict__["_deferred"] == ref.__dict__["_deferred"], what
    assert (got.__dict__["_parts_used"], got.__dict__["_fullest_tile"]) == (ref.__dict__["_parts_used"], ref.__dict__["_fullest_tile"]), what


def _assert_empty_plan(got, size, tile, what):
    """An empty range has no single build (``build_raw`` raises IndexError for it): the batch gives the plan of no events -- zero
    offsets, zero counts, and the work items ``ebos_plan_parts`` makes of those offsets (one per tile)."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip, event_plan

    n_tiles = -(-size[0] // tile[0]) * -(-size[1] // tile[1])
    assert (got.n, got.n_input, got.n_dropped) == (0, 0, 0) and got.key_offsets.numel() == n_tiles * tile[0] * tile[1] + 1, what
    assert not got.key_offsets.any() and not got.grp_offsets.any() and not got.__dict__["_counts"].any(), what
    ref = torch.empty_like(got.part_table)
    zeros = torch.zeros_like(got.key_offsets)
    n_cu = event_plan._n_cu(got.device)
    _hip.check(ebos.load_library().ebos_plan_parts(zeros.data_ptr(), size[0], size[1], tile[0], tile[1], n_cu,
                                                   event_plan.part_fixed_events(0, n_tiles, n_cu), ref.data_ptr(), _hip.stream_ptr()), "parts")
    assert torch.equal(got.part_table, ref), what


_CACHE = {}


def _device_recording(geom, t_dtype):
    key = (geom, np.dtype(t_dtype).name)
    if key not in _CACHE:
        size, tile = GEOMS[geom]
        cols, seg = _recording(size, tile, t_dtype)
        _CACHE[key] = (tuple(torch.from_numpy(c).cuda() for c in cols), seg)
    return _CACHE[key]


def _single(dev_cols, rng, size, direction, normalize, tile, deferred=True):
    import event_based_bos_amd as ebos

    a, b = rng
    return ebos.EventPlan.build_raw(*(c[a:b] for c in dev_cols), size, direction, normalize, tile=tile, deferred=deferred, emit="compact")


# every geometry, both tick widths, the three kinds of direction, normalisation on and off
CASES = [("64x96/32x32", np.int32, "first", True), ("64x96/32x32", np.int64, 0.3, False), ("100x150/32x64", np.int64, "middle", True),
         ("100x150/32x64", np.int32, "first", False), ("90x160/45x80", np.int32, 0.7, True), ("90x160/45x80", np.int64, "middle", False)]


@pytest.mark.parametrize("geom,t_dtype,direction,normalize", CASES)
def test_batched_plans_equal_the_single_builds_bit_for_bit(geom, t_dtype, direction, normalize):
    import event_based_bos_amd as ebos

    size, tile = GEOMS[geom]
    cols, seg = _device_recording(geom, t_dtype)
    singles = {}
    for name, ranges in _batches(seg).items():
        plans = ebos.EventPlan.build_raw_batch(*cols, ranges, size, direction, normalize, tile=tile, deferred=True)
        assert len(plans) == len(ranges)
        for k, (rng, got) in enumerate(zip(ranges, plans)):
            what = (geom, name, k, rng)
            if rng[0] == rng[1]:
                _assert_empty_plan(got, size, tile, what)
                continue
            if rng not in singles:
                singles[rng] = _single(cols, rng, size, direction, normalize, tile)
            _assert_same_plan(got, singles[rng], what)
    # the buffers are shared: the plans of one batch are views of one storage each
    plans = ebos.EventPlan.build_raw_batch(*cols, _batches(seg)["five"], size, direction, normalize, tile=tile)
    assert len({p.cdt.untyped_storage().data_ptr() for p in plans}) == 1 and len({p.key_offsets.untyped_storage().data_ptr() for p in plans}) == 1


@pytest.mark.parametrize("geom,t_dtype", [("64x96/32x32", np.int32), ("100x150/32x64", np.int64)])
def test_one_read_back_fills_the_facts_of_every_plan(geom, t_dtype):
    """``deferred=False``: dropped events (five in the OOB window), work items in use and the fullest tile of every plan, as the single
    builds' read-backs report them."""
    import event_based_bos_amd as ebos

    size, tile = GEOMS[geom]
    cols, seg = _device_recording(geom, t_dtype)
    ranges = [seg["OOB"], seg["HOT"], seg["TILE"], seg["B"]]
    plans = ebos.EventPlan.build_raw_batch(*cols, ranges, size, "middle", True, tile=tile, deferred=False)
    for k, (rng, got) in enumerate(zip(ranges, plans)):
        ref = _single(cols, rng, size, "middle", True, tile, deferred=False)
        _assert_same_plan(got, ref, (geom, k))
        assert got.__dict__["_parts_used"] is not None and got.__dict__["_fullest_tile"] is not None
        assert got.counts() == ref.counts()
    assert plans[0].n_dropped == 5 and plans[0].n == 295 and plans[1].__dict__["_fullest_tile"] >= 3000


def test_store_plans_equal_store_plan():
    import event_based_bos_amd as ebos

    size, tile = GEOMS["100x150/32x64"]
    (col, row, t, pol), seg = _recording(size, tile, np.int32, seed=3)
    store = ebos.data_loader.RawEventStore({"x": col, "y": row, "t": t, "p": pol.astype(bool)})
    windows = [seg["B"], seg["HOT"], (seg["A"][0] + 50, seg["A"][0] + 2050)]   # (not from index 0, out of order)
    plans = store.plans(windows, size, "first", True, tile=tile)
    for k, (wnd, got) in enumerate(zip(windows, plans)):
        _assert_same_plan(got, store.plan(wnd[0], wnd[1], size, "first", True, tile=tile, deferred=True, emit="compact"), k)
    with pytest.raises(IndexError):
        store.plans([seg["B"], (10, 10)], size, tile=tile)      # (an empty window, as RawEventStore.plan refuses it)


def test_batched_plans_run_the_slab_batch_and_the_dense_objective():
    import event_based_bos_amd as ebos

    size, tile = GEOMS["64x96/32x32"]
    cols, seg = _device_recording("64x96/32x32", np.int32)
    ranges = [seg["A"], seg["B"], seg["HOT"]]
    batched = ebos.EventPlan.build_raw_batch(*cols, ranges, size, "first", True, tile=tile)
    singles = [_single(cols, r, size, "first", True, tile) for r in ranges]
    g = torch.Generator().manual_seed(1)
    flows = [(torch.rand((2,) + size, generator=g) * 6 - 3).cuda() for _ in ranges]
    sb, ss = ebos.SlabBatch(batched, flows), ebos.SlabBatch(singles, flows)
    vb, vs = sb.run().clone(), ss.run().clone()
    assert torch.equal(sb.iwes, ss.iwes) and torch.equal(vb, vs) and float(vb.min()) > 0
    v1, g1 = batched[0].variance_and_grad_dense(flows[0])
    v2, g2 = singles[0].variance_and_grad_dense(flows[0])
    assert torch.equal(v1, v2) and torch.equal(g1, g2) and float(g1.abs().max()) > 0


@pytest.mark.parametrize("geom,tile", [("64x96/32x32", (264, 32)), ("100x150/32x64", (1, 1))])
def test_a_tile_outside_the_lds_sort_is_built_window_by_window(geom, tile):
    """A tile higher than 256 rows (refused by the Python layer) or a grid of more bins than the LDS histogram holds (the whole call
    answers EBOS_ERR_UNSUPPORTED): the plans ``build_raw`` makes of the windows one by one.  That route is the general build, whose
    order inside a source pixel is not canonical: offsets, counts and work items are compared exactly, the events as sets."""
    import event_based_bos_amd as ebos

    size = GEOMS[geom][0]
    cols, seg = _device_recording(geom, np.int32)
    ranges = [seg["B"], seg["OOB"]]
    plans = ebos.EventPlan.build_raw_batch(*cols, ranges, size, "first", True, tile=tile)
    for rng, got in zip(ranges, plans):
        ref = _single(cols, rng, size, "first", True, tile)
        assert not got.lean and got.compact == ref.compact and (got.n, got.n_input, got.tile) == (ref.n, ref.n_input, ref.tile)
        assert torch.equal(got.key_offsets, ref.key_offsets) and torch.equal(got.part_table, ref.part_table)
        assert torch.equal(got.__dict__["_counts"], ref.__dict__["_counts"])
        assert torch.equal(torch.sort(_bits(got.dt))[0], torch.sort(_bits(ref.dt))[0])
        if ref.compact:
            assert torch.equal(got.grp_offsets, ref.grp_offsets) and torch.equal(got.cpix, ref.cpix)


def _cfg():
    return yaml.safe_load(open(os.path.join(ROOT, "configs", "cmax_hot_plate1.yaml")))["solver"]


def _moving_points(h, w, n_points, per_point, v, seed):
    rs = np.random.RandomState(seed)
    p0 = np.stack([rs.uniform(8, h - 16, n_points), rs.uniform(8, w - 16, n_points)], 1)
    t = rs.uniform(0, 1, (n_points, per_point))
    x, y = np.rint(p0[:, None, 0] + t * v[0]).reshape(-1), np.rint(p0[:, None, 1] + t * v[1]).reshape(-1)
    keep = (x >= 0) & (x < h) & (y >= 0) & (y < w)
    return x[keep], y[keep]


@pytest.mark.parametrize("model", ["patch", "2dof"])
def test_pipeline_with_batched_ingest_reproduces_the_default_run(model):
    """Four windows through ``WindowPipeline`` with ``batch_ingest`` on and off: the plans are the same bits, so flows, loss histories,
    dropped events and the way every window ran are equal.  (The smallest sensors and solver settings of the pipeline's own tests.)"""
    import event_based_bos_amd as ebos

    cfg = _cfg()
    if model == "patch":
        h, w = 96, 128
        rs = np.random.RandomState(11)
        cols, rows, ts, bounds = [], [], [], [0]
        for k in range(4):
            x, y = _moving_points(h, w, 400, 30, np.array([3.0 + k, -2.0 + 0.5 * k]), seed=20 + k)
            if k == 2:   # (three events outside the sensor: dropped_events)
                x[:3] = h + 1
            rows.append(x); cols.append(y)
            ts.append(np.sort(rs.randint(0, 20000, len(x))) + 1_000_000 + 30000 * k)
            bounds.append(bounds[-1] + len(x))
        data = {"x": np.concatenate(cols), "y": np.concatenate(rows), "t": np.concatenate(ts)}
        data["p"] = rs.randint(0, 2, len(data["t"])).astype(bool)
        windows = [(bounds[k], bounds[k + 1]) for k in range(4)]
        cfg.update(patch={"size": [24, 32], "sliding_window": [24, 32]}, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.01},
                   iwe={"method": "bilinear_vote", "blur_sigma": 0}, optimizer={"method": "Adam", "n_iter": 36, "parameters": {"lr": 0.2}})
    else:
        h, w = 260, 346
        rs = np.random.RandomState(9)
        n = 30_000
        data = {"x": rs.randint(0, w, n * 4).astype(np.int16), "y": rs.randint(0, h, n * 4).astype(np.int16),
                "t": np.sort(rs.randint(0, 32000, n * 4)).astype(np.int32) + 1_000_000, "p": rs.randint(0, 2, n * 4).astype(bool)}
        windows = [(i * n, (i + 1) * n) for i in range(4)]
        cfg.update(motion_model="2d-translation", parameters=["trans_x", "trans_y"], cost_with_weight={"image_variance": 1.0},
                   iwe={"method": "bilinear_vote", "blur_sigma": 0.0}, optimizer={"method": "Adam", "n_iter": 50, "parameters": {"lr": 0.05}})
    store = ebos.data_loader.RawEventStore(data)
    solver = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    plain = ebos.solver.WindowPipeline(solver, n_concurrent=3)
    assert plain.batch_ingest is False
    flows = plain.run(store, windows)
    batched = ebos.solver.WindowPipeline(solver, n_concurrent=3, batch_ingest=True)
    assert batched.batch_ingest is True and batched.tile == plain.tile
    flows_b = batched.run(store, windows)
    assert len(flows_b) == 4
    for k in range(4):
        np.testing.assert_array_equal(flows_b[k], flows[k])
        np.testing.assert_array_equal(np.array(batched.histories[k]), np.array(plain.histories[k]))
    assert batched.dropped_events == plain.dropped_events and batched.window_modes == plain.window_modes
    assert batched.resident_fallbacks == plain.resident_fallbacks
    if model == "patch":
        assert plain.dropped_events == [0, 0, 3, 0]
