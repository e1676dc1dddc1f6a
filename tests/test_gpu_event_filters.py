"""The event filters on the MI355X (csrc/event_filters.hip through event_based_bos_amd/event_filters.py): bit-identical to the
reference's loops on its own outputs (tests/golden/golden_filters.npz) through the numpy and the device-tensor API, raw columns
== float64 events, independent of atomic order, exact at 2 M events (against the numpy restatement tests/_filter_ref.py), and
wired through SolverBase.preprocess and WindowPipeline."""
import json
import os

import numpy as np
import pytest
import torch

from _filter_ref import baf_numpy, hot_numpy, load_golden_filters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (260, 346)


@pytest.fixture(scope="module")
def golden():
    return load_golden_filters(os.path.join(ROOT, "tests", "golden", "golden_filters.npz"))


def _cases(g, prefix):
    return sorted({k[:-len("_params")] for k in g if k.startswith(prefix) and k.endswith("_params")})


def test_baf_matches_the_reference_bit_for_bit(golden):
    from event_based_bos_amd import event_filters as F

    for c in _cases(golden, "baf_"):
        ev, m0, (dt, k, s) = golden[c + "_events"], golden[c + "_m0"], golden[c + "_params"]
        tm = m0.copy()
        kept, m = F.continuous_background_activity_filter(ev, HW, dt, int(k), int(s), time_map=tm)
        assert isinstance(kept, np.ndarray) and m is tm, c
        np.testing.assert_array_equal(kept, golden[c + "_kept"], err_msg=c)
        np.testing.assert_array_equal(tm, golden[c + "_map"], err_msg=c)
        dev = torch.from_numpy(ev).cuda()
        kept_t, m_t = F.continuous_background_activity_filter(dev, HW, dt, int(k), int(s), time_map=torch.from_numpy(m0).cuda())
        assert kept_t.is_cuda and m_t.is_cuda and kept_t.dtype == dev.dtype
        np.testing.assert_array_equal(kept_t.cpu().numpy(), golden[c + "_kept"], err_msg=c)
        np.testing.assert_array_equal(m_t.cpu().numpy(), golden[c + "_map"], err_msg=c)
        if not m0.any():
            np.testing.assert_array_equal(F.background_activity_filter(ev, HW, dt, int(k), int(s)), golden[c + "_kept"])


def test_hot_matches_the_reference_bit_for_bit(golden):
    from event_based_bos_amd import event_filters as F

    for c in ("hot_int", "hot_int_f32", "hot_frac"):
        ev, th = golden[c + "_events"], golden[c + "_params"][0]
        np.testing.assert_array_equal(F.hot_pixel_filter(ev, HW, th), golden[c + "_kept"], err_msg=c)
        out = F.hot_pixel_filter(torch.from_numpy(ev).cuda(), HW, th)
        assert out.is_cuda
        np.testing.assert_array_equal(out.cpu().numpy(), golden[c + "_kept"], err_msg=c)


@pytest.mark.parametrize("cont", [0, 1])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_event_filter_sequence_matches_the_reference(golden, cont, as_tensor):
    from event_based_bos_amd.event_filters import EventFilter

    cfg = json.loads(golden[f"seq_{cont}_config"].tobytes().decode())
    ef = EventFilter(HW, cfg)
    assert ef.filters == ["CROP", "BAF", "HOT"]
    for k in range(3):
        w = golden[f"seq_{cont}_w{k}_in"]
        out = ef.process(torch.from_numpy(w).cuda() if as_tensor else w)
        out = out.cpu().numpy() if as_tensor else out
        np.testing.assert_array_equal(out, golden[f"seq_{cont}_w{k}_out"], err_msg=f"window {k}")
        m = np.zeros(HW) if ef.time_map is None else ef.time_map.cpu().numpy()
        np.testing.assert_array_equal(m, golden[f"seq_{cont}_w{k}_map"], err_msg=f"window {k}")


def _window(n, H, W, seed, n_hot=0, hot_count=0, clusters=0):
    """Integer events: uniform noise + events clustered around moving points + hot pixels; times partly out of order."""
    rs = np.random.RandomState(seed)
    x, y = rs.randint(0, H, n), rs.randint(0, W, n)
    if clusters:
        m = n // 2
        c = rs.randint(0, clusters, m)
        cx, cy = rs.uniform(0, H, clusters), rs.uniform(0, W, clusters)
        x[:m] = np.clip(cx[c] + rs.normal(0, 3, m), 0, H - 1).astype(int)
        y[:m] = np.clip(cy[c] + rs.normal(0, 3, m), 0, W - 1).astype(int)
    t = np.sort(rs.randint(0, 50_000, n)).astype(np.int64)
    sw = rs.choice(n - 3, n // 20, replace=False)
    t[sw], t[sw + 2] = t[sw + 2], t[sw].copy()
    if n_hot:
        hp = rs.randint(0, [H, W], (n_hot, 2))
        idx = rs.choice(n, n_hot * hot_count, replace=False)
        x[idx], y[idx] = np.repeat(hp[:, 0], hot_count), np.repeat(hp[:, 1], hot_count)
    p = rs.randint(0, 2, n)
    return x, y, t, p


def _aos(x, y, t, p):
    return np.stack([x, y, t / 1e6, p], 1).astype(np.float64)


def test_raw_columns_and_float64_events_give_the_same_masks_and_maps():
    from event_based_bos_amd import event_filters as F

    H, W = HW
    x, y, t, p = _window(120_000, H, W, 3, n_hot=10, hot_count=200, clusters=40)
    dev = torch.device("cuda")
    raw = F._Window(raw=(torch.from_numpy(y.astype(np.int16)).to(dev), torch.from_numpy(x.astype(np.int16)).to(dev),
                         torch.from_numpy(t.astype(np.int32)).to(dev), torch.from_numpy(p.astype(np.uint8)).to(dev)))
    aos = F._Window(events=torch.from_numpy(_aos(x, y, t, p)).to(dev))
    got = []
    for win in (raw, aos):
        ch = F._Chain(win, HW)
        m = ch.baf(0.002, 1, 1, None)
        baf_mask = ch.mask.clone()
        ch.hot(10)
        got.append((baf_mask.cpu().numpy(), m.cpu().numpy(), ch.mask.cpu().numpy()))
        out = ch.compact()
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)
    kept, m_ref = baf_numpy(_aos(x, y, t, p), HW, 0.002, 1, 1)
    np.testing.assert_array_equal(got[0][1], m_ref)
    np.testing.assert_array_equal(_aos(x, y, t, p)[got[0][0].astype(bool)], kept)
    np.testing.assert_array_equal(out.events.cpu().numpy(), hot_numpy(kept, HW, 10))


def test_a_30000_event_pixel_gives_the_same_result_every_run():
    from event_based_bos_amd import event_filters as F

    H, W = HW
    x, y, t, p = _window(200_000, H, W, 5, n_hot=1, hot_count=30_000)
    ev = _aos(x, y, t, p)
    a = F.continuous_background_activity_filter(torch.from_numpy(ev).cuda(), HW, 0.001, 2, 3)
    b = F.continuous_background_activity_filter(torch.from_numpy(ev).cuda(), HW, 0.001, 2, 3)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    kept, m = baf_numpy(ev, HW, 0.001, 2, 3)
    np.testing.assert_array_equal(a[0].cpu().numpy(), kept)
    np.testing.assert_array_equal(a[1].cpu().numpy(), m)


def test_two_million_events_at_1280x720_match_the_restatement():
    from event_based_bos_amd.event_filters import EventFilter

    H, W = 720, 1280
    x, y, t, p = _window(2_000_000, H, W, 9, n_hot=40, hot_count=500, clusters=300)
    ev = _aos(x, y, t, p)
    ef = EventFilter((H, W), {"filters": ["BAF", "HOT"], "parameters": {"BAF_dt": 0.0005, "BAF_ksize": 1, "BAF_num_support_event": 1,
                                                                         "BAF_continuous_update": True, "HOT_thresh": 10}})
    got = ef.process(torch.from_numpy(ev).cuda()).cpu().numpy()
    kept, m = baf_numpy(ev, (H, W), 0.0005, 1, 1)
    want = hot_numpy(kept, (H, W), 10)
    assert 0 < len(want) < len(kept) < len(ev)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ef.time_map.cpu().numpy(), m)


def _filter_section(roi=None, cont=True):
    p = {"BAF_dt": 0.004, "BAF_ksize": 1, "BAF_num_support_event": 1, "BAF_continuous_update": cont, "HOT_thresh": 10}
    if roi is not None:
        p.update(roi)
    return {"filters": ["BAF", "HOT"], "parameters": p}


def _cm_solver(shape, filter_section):
    import yaml

    import event_based_bos_amd as ebos

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cmax_hot_plate1.yaml")))["solver"]
    cfg.pop("filter", None)
    cfg.update(patch={"size": [32, 32], "sliding_window": [32, 32]}, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.01},
               iwe={"method": "bilinear_vote", "blur_sigma": 0}, optimizer={"method": "Adam", "n_iter": 20, "parameters": {"lr": 0.2}})
    if filter_section is not None:
        cfg["filter"] = filter_section
    return ebos.solver.collections["contrast_maximization"](shape, shape, solver_config=cfg)


def test_solver_preprocess_runs_the_listed_filters(golden):
    cfg = json.loads(golden["seq_1_config"].tobytes().decode())
    s = _cm_solver(HW, cfg)
    plain = _cm_solver(HW, {"parameters": {k: cfg["parameters"][k] for k in ("xmin", "xmax", "ymin", "ymax")}})
    assert s.filter_set is not None and plain.filter_set is None
    for k in range(3):
        w = golden[f"seq_1_w{k}_in"]
        out, period = s.preprocess(w)
        np.testing.assert_array_equal(out, golden[f"seq_1_w{k}_out"], err_msg=f"window {k}")
        cropped, period_plain = plain.preprocess(w)
        assert period == period_plain                      # (the period of the cropped window, as before)
        np.testing.assert_array_equal(s.filter_set.time_map.cpu().numpy(), golden[f"seq_1_w{k}_map"])
    # a config without a filters list: exactly the crop of before
    w = golden["seq_1_w0_in"]
    x0, x1, y0, y1 = plain.roi
    np.testing.assert_array_equal(plain.preprocess(w)[0], w[(w[:, 0] >= x0) & (w[:, 0] < x1) & (w[:, 1] >= y0) & (w[:, 1] < y1)])


def _recording(H, W, n_windows, seed):
    cols, rows, ts, ps, bounds = [], [], [], [], [0]
    for k in range(n_windows):
        x, y, t, p = _window(60_000, H, W, seed + k, n_hot=6, hot_count=40, clusters=200)
        t = np.sort(t) + 1_000_000 + 60_000 * k
        rows.append(x); cols.append(y); ts.append(t); ps.append(p)
        bounds.append(bounds[-1] + len(t))
    data = {"x": np.concatenate(cols).astype(np.int16), "y": np.concatenate(rows).astype(np.int16),
            "t": np.concatenate(ts).astype(np.int32), "p": np.concatenate(ps).astype(np.uint8)}
    return data, [(bounds[k], bounds[k + 1]) for k in range(n_windows)]


def test_window_pipeline_filters_every_window():
    import event_based_bos_amd as ebos
    from event_based_bos_amd.event_filters import EventFilter
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    H, W = HW
    data, windows = _recording(H, W, 5, 41)
    store = ebos.data_loader.RawEventStore(data)
    sec = _filter_section()
    solver = _cm_solver(HW, sec)
    pipe = ebos.solver.WindowPipeline(solver, n_concurrent=2)
    assert pipe.filters is not None and pipe.filters.filters == ["BAF", "HOT"]
    flows = pipe.run(store, windows)

    # the same filters, window by window in list order, on the host-side reference format -> a store of the kept events
    ef = EventFilter(HW, sec)
    kept_cols, bounds = {k: [] for k in "xytp"}, [0]
    for (a, b) in windows:
        out = ef.process(store.load_event(a, b))
        kept_cols["x"].append(out[:, 1]); kept_cols["y"].append(out[:, 0]); kept_cols["p"].append(out[:, 3])
        kept_cols["t"].append(np.rint(out[:, 2] * 1e6))
        bounds.append(bounds[-1] + len(out))
    pre = ebos.data_loader.RawEventStore({"x": np.concatenate(kept_cols["x"]).astype(np.int16),
                                          "y": np.concatenate(kept_cols["y"]).astype(np.int16),
                                          "t": np.concatenate(kept_cols["t"]).astype(np.int32),
                                          "p": np.concatenate(kept_cols["p"]).astype(np.uint8)})
    pre_windows = [(bounds[k], bounds[k + 1]) for k in range(len(windows))]
    assert all(b - a < wb - wa for (a, b), (wa, wb) in zip(pre_windows, windows))

    # plan arrays of a filtered window == those of build_raw on the filtered columns
    pipe.filters.reset()
    for k, wnd in enumerate(windows[:2]):
        plan, cols = pipe._ingest(store, wnd)
        ref = ebos.EventPlan.build_raw(*pre.load_raw(*pre_windows[k]), HW, solver.warp_direction, True, tile=pipe.tile,
                                       ticks_per_second=1e6, deferred=True, emit="compact")
        assert torch.equal(plan.key_offsets, ref.key_offsets) and torch.equal(plan.grp_offsets, ref.grp_offsets)
        used = 4 * int(ref.grp_offsets[-1])     # (the slots the lean plan fills; the tail of its buffers is capacity)
        assert torch.equal(plan.cpix[:used], ref.cpix[:used])
        assert torch.equal(plan.cdt[:used].view(torch.int32), ref.cdt[:used].view(torch.int32))

    plain = ebos.solver.WindowPipeline(_cm_solver(HW, None), n_concurrent=2)
    assert plain.filters is None
    want = plain.run(pre, pre_windows)
    for k in range(len(windows)):
        np.testing.assert_array_equal(flows[k], want[k])

    # a resident launch that ends early: its window is solved again from the events it was filtered to the first time
    orig, calls = FusedPatchLoop.enqueue_resident, {"n": 0}

    def ends_early(self, n_iter, spin_timeout_s=2.0):
        calls["n"] += 1
        if calls["n"] == 2:
            return torch.full((1,), 2, dtype=torch.int32, device=self.plan.device)
        return orig(self, n_iter, spin_timeout_s)

    FusedPatchLoop.enqueue_resident = ends_early
    try:
        flows_fb = pipe.run(store, windows)
    finally:
        FusedPatchLoop.enqueue_resident = orig
    if pipe.resident:
        assert pipe.resident_fallbacks == [1]
    for k in range(len(windows)):
        np.testing.assert_array_equal(flows_fb[k], flows[k])


def test_unsupported_ranges_and_bad_events_raise():
    from event_based_bos_amd import event_filters as F

    ev = _aos(*_window(5000, HW[0], HW[1], 2))
    with pytest.raises(NotImplementedError):
        F.background_activity_filter(ev, HW, 0.001, ksize=8)
    with pytest.raises(NotImplementedError):
        F.background_activity_filter(ev, HW, 0.001, ksize=1, num_support_event=16)
    bad = ev.copy()
    bad[7, 0] = -1.5
    with pytest.raises(ValueError):
        F.background_activity_filter(bad, HW, 0.001)
    bad = ev.copy()
    bad[9, 1] = HW[1]
    with pytest.raises(ValueError):
        F.hot_pixel_filter(bad, HW, 10)
    with pytest.raises(IndexError):   # a 1-pixel neighbourhood cannot hold 2 support values (the reference's IndexError)
        F.background_activity_filter(ev, HW, 0.001, ksize=0, num_support_event=1)
    # ... but a corner is only an error when an event lands there
    inner = ev[(ev[:, 0] > 0) & (ev[:, 0] < HW[0] - 1) & (ev[:, 1] > 0) & (ev[:, 1] < HW[1] - 1)]
    kept, _ = F.continuous_background_activity_filter(inner, HW, 0.001, 1, 8)
    np.testing.assert_array_equal(kept, baf_numpy(inner, HW, 0.001, 1, 8)[0])
    edge = inner.copy()
    edge[3, :2] = 0
    with pytest.raises(IndexError):
        F.continuous_background_activity_filter(edge, HW, 0.001, 1, 8)
