"""The recording evaluator on the GPU (event_based_bos_amd/evaluation.py, csrc/window_ingest.hip).

1. ``window_ingest_raw_batch`` against the existing converter, bit for bit: the polarity image, the event mask, the count and the
   period of every window of a batch (empty, one event, 1 000, about 1 M; overlapping; all-positive, all-negative; a pixel with more
   than 65 535 events), with and without CROP and removal rectangle, twice.
2. ``estimate_batch_prepared`` == ``estimate_batch`` on the same windows handed over as numpy arrays: flows, histories, parameters
   and numpy's RandomState, with ``np.array_equal``.
3. ``RecordingEvaluator`` == the reference driver's loop written out over the existing public calls, on a synthetic recording:
   error dicts, timestamps and the three text files.
4. The masked EPE the evaluator reports is the loop's.

Every comparison is exact (``np.array_equal`` / equal file contents): both sides run the same kernels on the same values, the counts
are integers, and the error reductions are per item with a fixed order that does not depend on the batch size.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_cases as CP  # noqa: E402
import _gml_dep_cases as CD  # noqa: E402

pytestmark = pytest.mark.gpu

TPS = 1e6


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as ebos
    return ebos


# ------------------------------------------------------------------------------------------------ 1. the ingest kernel
N_STORE = 1_200_000
HOT = 70_000          # events on one pixel: more than a 16-bit counter holds


def _store_columns(H, W, roi, seed=3):
    """Raw columns of N_STORE events: random pixels and polarities, one hot pixel inside the CROP rectangle, a block of positive
    events and a block of negative ones at the end."""
    rs = np.random.RandomState(seed)
    x = rs.randint(0, W, N_STORE).astype(np.int16)
    y = rs.randint(0, H, N_STORE).astype(np.int16)
    p = rs.randint(0, 2, N_STORE).astype(bool)
    t = np.sort(rs.randint(1000, 3_000_000, N_STORE)).astype(np.int32)
    hot = rs.choice(1_000_000, HOT, replace=False)
    r0, r1, c0, c1 = roi
    y[hot], x[hot], p[hot] = r1 - 3, c1 - 2, True   # (outside the removal rectangle of the cases below; one polarity)
    p[1_100_000:1_150_000] = True
    p[1_150_000:] = False
    return x, y, t, p


RANGES = [(0, 0), (5, 6), (100, 1100), (0, 1_000_000), (500_000, 1_200_000), (1_100_000, 1_150_000), (1_150_000, 1_200_000),
          (700, 700), (999_990, 1_000_010)]
INGEST_CASES = {
    "260_plain": ((260, 346), (0, 260, 86, 260), False, False),
    "260_roi": ((260, 346), (0, 260, 86, 260), True, False),
    "260_roi_remove": ((260, 346), (0, 260, 86, 260), True, True),
    "260_remove": ((260, 346), (0, 260, 86, 260), False, True),
    "720_plain": ((720, 1280), (0, 720, 320, 960), False, False),
    "720_roi_remove": ((720, 1280), (0, 720, 320, 960), True, True),
}


def _remove_rect(shape):
    return (0, 120, 990, 1050) if shape[1] > 1050 else (10, 120, 100, 180)


@pytest.mark.parametrize("name", sorted(INGEST_CASES))
def test_ingest_equals_the_converter(ebos, name):
    from event_based_bos_amd.evaluation import window_ingest_raw_batch
    from event_based_bos_amd.solver.base import SolverBase
    from event_based_bos_amd.utils import remove_event

    shape, roi, use_roi, use_rm = INGEST_CASES[name]
    H, W = shape
    x, y, t, p = _store_columns(H, W, roi)
    store = ebos.RawEventStore({"x": x, "y": y, "t": t, "p": p})
    cols = store.load_raw(0, N_STORE)
    rm = _remove_rect(shape) if use_rm else None
    got = window_ingest_raw_batch(cols, RANGES, shape, roi if use_roi else None, rm, TPS)
    again = window_ingest_raw_batch(cols, RANGES, shape, roi if use_roi else None, rm, TPS)
    for a, b in ((got.pol, again.pol), (got.mask, again.mask), (got.count, again.count), (got.t_min, again.t_min),
                 (got.t_max, again.t_max)):
        assert torch.equal(a, b)                                               # two runs are identical
    cfg = {"filter": {"parameters": dict(zip(("xmin", "xmax", "ymin", "ymax"), roi))}} if use_roi else {}
    base = SolverBase(shape, (roi[1] - roi[0], roi[3] - roi[2]), None, cfg)
    imager = ebos.EventImageConverter(shape)
    count, period = got.count.cpu().numpy(), got.period.cpu().numpy()
    seen_hot = False
    for b, (lo, hi) in enumerate(RANGES):
        ev = store.load_event(lo, hi) if hi > lo else np.zeros((0, 4))
        if rm is not None:
            ev = remove_event(ev, *rm)
        kept, want_period = base.preprocess(ev)
        want_pol = torch.from_numpy(imager.create_image_from_events_numpy(kept, method="polarity", sigma=0)).reshape(2, H, W) \
            if len(kept) else torch.zeros((2, H, W), dtype=torch.float64)
        want_mask = torch.from_numpy(np.asarray(imager.create_eventmask(kept))).reshape(H, W) if len(kept) else \
            torch.zeros((H, W), dtype=torch.bool)
        assert torch.equal(got.pol[b].cpu(), want_pol), (name, b)
        assert torch.equal(got.mask[b].cpu().bool(), want_mask), (name, b)
        assert count[b] == len(kept), (name, b)
        assert np.array_equal(period[b], np.float64(want_period)), (name, b, period[b], want_period)
        if len(kept):
            assert torch.equal(got.events(b).cpu(), torch.from_numpy(kept)), (name, b)
        seen_hot |= float(want_pol.max()) > 65535
    assert seen_hot
    assert float(got.pol[5, 1].sum()) == 0 and float(got.pol[6, 0].sum()) == 0 and count[5] > 0 and count[6] > 0
    assert count[0] == 0 and count[7] == 0 and period[0] == 0.0


def test_ingest_refuses_fractional_columns(ebos):
    from event_based_bos_amd.evaluation import window_ingest_raw_batch

    z = torch.zeros(4, device="cuda")
    with pytest.raises(ValueError):
        window_ingest_raw_batch((z, z, z.int(), z.to(torch.uint8)), [(0, 4)], (8, 8))


# ------------------------------------------------------------------------------------------------ 2. the prepared solver path
KINDS = {"pyramid": ("generative_patch_pyramid", CP), "dependent": ("generative_patch_dependent", CD)}
PREPARED = [("pyramid", "yaml_260"), ("pyramid", "evhist_128"), ("dependent", "yaml_260"), ("dependent", "evhist_128"),
            ("dependent", "thres_128")]


def _solver(ebos, kind, name, n_iter):
    key, cases = KINDS[kind]
    c = cases.CASES[name]
    cfg = cases.solver_config(name)
    cfg["optimizer"]["n_iter"] = n_iter
    return ebos.solver.collections[key](c["shape"], c["shape"], {}, cfg)


def _left_behind(kind, s, flows):
    out = {"flow": np.asarray(flows)}
    for i, h in enumerate(s.histories):
        out.update({f"hist{i}_{k}": np.array(v) for k, v in h.items()})
    if kind == "pyramid":
        for i, d in enumerate(s.params_per_scale_batch):
            out.update({f"x{i}_{k}": v for k, v in d.items()})
        out.update({f"last_x_{k}": v for k, v in s.params_per_scale.items()})
    else:
        out.update({f"x{i}": v for i, v in enumerate(s.params_batch)})
        out.update({f"sel{i}": v for i, v in enumerate(s.estimate_indices_batch)})
        out["last_x"], out["last_sel"] = s.params, s.estimate_indices
    out.update({"last_hist_" + k: np.array(v) for k, v in s.cost_func.get_history().items()})
    out["iter_cnt"] = np.array(s.iter_cnt)
    return out


@pytest.mark.parametrize("kind,name", PREPARED)
def test_prepared_path_equals_estimate_batch(ebos, kind, name):
    from event_based_bos_amd.evaluation import window_ingest_raw_batch

    cases = KINDS[kind][1]
    c = cases.CASES[name]
    H, W = c["shape"]
    frame, ev0 = cases.case_inputs(name)
    make = CD.clustered_events if c.get("clustered") else CP.synth_events
    sizes = [len(ev0), len(ev0) // 2 + 7, len(ev0) // 3]
    wins = [ev0] + [make(n, H, W, 700 + 13 * i + c["seed"]) for i, n in enumerate(sizes[1:])]
    # the same windows as raw columns: integer pixels, microsecond ticks
    ticks = [np.round(w[:, 2] * TPS).astype(np.int32) for w in wins]
    wins = [np.stack([w[:, 0], w[:, 1], tk / TPS, w[:, 3]], axis=1) for w, tk in zip(wins, ticks)]
    store = ebos.RawEventStore({"x": np.concatenate([w[:, 1] for w in wins]).astype(np.int16),
                                "y": np.concatenate([w[:, 0] for w in wins]).astype(np.int16),
                                "t": np.concatenate(ticks), "p": np.concatenate([w[:, 3] for w in wins]).astype(bool)})
    edges = np.concatenate([[0], np.cumsum([len(w) for w in wins])])
    ranges = [(int(edges[i]), int(edges[i + 1])) for i in range(len(wins))]
    for i, (lo, hi) in enumerate(ranges):
        assert np.array_equal(store.load_event(lo, hi), wins[i])
    frames = [frame, frame * 0.5 + 3.0, frame[::-1].copy()]
    n_iter = 24

    a = _solver(ebos, kind, name, n_iter)
    np.random.seed(11)
    want = _left_behind(kind, a, a.estimate_batch(wins, frames=frames, background=frame, max_batch=2))
    state_a = np.random.get_state()

    b = _solver(ebos, kind, name, n_iter)
    prepared = window_ingest_raw_batch(store.load_raw(0, len(store)), ranges, (H, W), None, None, TPS)
    np.random.seed(11)
    got = _left_behind(kind, b, b.estimate_batch_prepared(prepared, frames=frames, background=frame, max_batch=2))
    state_b = np.random.get_state()

    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (kind, name, k)
    assert state_a[0] == state_b[0] and np.array_equal(state_a[1], state_b[1]) and state_a[2:] == state_b[2:]
    dev = b.estimate_batch_prepared(prepared, frames=frames, background=frame, device_out=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and tuple(dev.shape) == (3, 2, H, W)


# ------------------------------------------------------------------------------------------------ 3. the evaluator
def _recording(ebos, tmp, shape, n_frames, events_per_interval, homography=True):
    from event_based_bos_amd.evaluation import synthetic_recording

    ev_path, fr_path, tr_path, stamps = synthetic_recording(str(tmp), shape, n_frames, events_per_interval, seed=5,
                                                            hot_pixel=(shape[0] // 2, shape[1] - 40))
    hom = np.array([[1.0, 0.002, 0.4], [-0.001, 1.0, 0.3], [0.0, 0.0, 1.0]]) if homography else None
    return ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path, hom, shape if homography else None), stamps


def _config(shape, roi, solver_method, n_iter, stamps, method="opencv_flow", filters=None, dt=1, remove_nose=False, n_events=None):
    from event_based_bos_amd.utils import propagate_config

    H, W = shape
    solver = copy.deepcopy(CP.solver_config("yaml_128"))
    solver["method"] = solver_method
    solver["optimizer"]["n_iter"] = n_iter
    solver["filter"] = {"filters": filters, "parameters": {"BAF_continuous_update": True, "BAF_dt": 0.005, "BAF_ksize": 1,
                                                             "BAF_num_support_event": 1, "HOT_thresh": 10}}
    solver["patch_eklt"] = {"patch_size": 8, "sliding_window": 8, "do_event_thresholding": False, "event_thres": 8}
    cfg = {"common_params": {"n_frames": dt, "xmin": roi[0], "xmax": roi[1], "ymin": roi[2], "ymax": roi[3]},
           "data": {"height": H, "width": W, "remove_nose": remove_nose},
           "estimation_method": "solver", "method": method,
           "evaluation": {"metrics": ["flow"], "time_list": [[float(stamps[0]) + 0.004, float(stamps[-1]) + 0.004]]},
           "params_opencv_flow": {"flags": 0, "iterations": 3, "levels": 3, "poly_n": 5, "poly_sigma": 1.2, "pyr_scale": 0.5,
                                  "winsize": 10},
           "solver": solver}
    if n_events is not None:
        cfg["data"]["n_events_per_batch"] = n_events
    return propagate_config(cfg)


class _Viz(object):
    def __init__(self, save_dir):
        self.save_dir = str(save_dir)
        os.makedirs(self.save_dir, exist_ok=True)


def _count_solver_class():
    """A solver without a prepared path (the evaluator drives it through ``preprocess`` + ``estimate``): its flow is a fixed
    function of the window's polarity counts, so two runs agree bit for bit."""
    from event_based_bos_amd.solver.base import SolverBase

    class CountSolver(SolverBase):
        def estimate(self, events, *args, **kwargs):
            img = self.orig_imager.create_image_from_events_numpy(np.asarray(events), method="polarity", sigma=0)
            return np.stack([0.1 * (img[0] - img[1]), 0.025 * (img[0] + img[1])])

    return CountSolver


def _make_solver(ebos, cfg, save_dir):
    d = cfg["data"]
    if cfg["solver"]["method"] == "count":
        return _count_solver_class()((d["height"], d["width"]), (d["crop_height"], d["crop_width"]), {}, cfg["solver"], _Viz(save_dir))
    key = {"patch_eklt_pyramid2": "generative_patch_pyramid", "patch_eklt_dependent": "generative_patch_dependent"}[cfg["solver"]["method"]]
    return ebos.solver.collections[key]((d["height"], d["width"]), (d["crop_height"], d["crop_width"]), {}, cfg["solver"], _Viz(save_dir))


def _driver_loop(ebos, cfg, events, frames, solv):
    """``evaluate_per_frames`` of the reference driver over the existing public calls, one window at a time."""
    from event_based_bos_amd import evaluation as E
    from event_based_bos_amd.frame_flow import FrameFlowEstimator
    from event_based_bos_amd.utils import remove_event

    common, data = cfg["common_params"], cfg["data"]
    cropped = (data["crop_height"], data["crop_width"])
    dt = cfg["evaluation"]["dt"]
    n_events = data.get("n_events_per_batch")
    max_dt = data.get("max_time_per_event_batch")
    estimator = FrameFlowEstimator(None)
    im0, _ = frames.load_image(0)
    frame0 = ebos.validate_image(im0, common)
    out = {"e0": [], "e1": [], "ts": []}
    i_frame = 0
    for lo_t, hi_t in cfg["evaluation"]["time_list"]:
        ind_start = frames.time_to_image_index(lo_t) + 1
        ind_end = frames.time_to_image_index(hi_t) - dt
        for i1 in range(ind_start, ind_end):
            i2 = i1 + dt
            im1, t1 = frames.load_image(i1)
            im2, t2 = frames.load_image(i2)
            frame1, frame2 = ebos.validate_image(im1, common), ebos.validate_image(im2, common)
            if frame1.shape != cropped or frame2.shape != cropped:
                continue
            gt_flow = estimator.estimate(cfg["method"], frame0, frame1, frame2, cfg)
            ind1, ind2 = events.time_to_index(t1), events.time_to_index(t2)
            events.load_event(max(ind1, 0), min(ind2, len(events)))
            if max_dt is not None and t2 - t1 > max_dt:
                t2 = t1 + max_dt
                ind1, ind2 = events.time_to_index(t1), events.time_to_index(t2)
            if n_events is not None:
                if ind2 - ind1 < n_events:
                    insufficient = n_events - (ind2 - ind1)
                    ind1 -= insufficient // 2
                    ind2 += insufficient // 2
                elif ind2 - ind1 > n_events:
                    ind1 = ind2 - n_events
            batch = events.load_event(max(ind1, 0), min(ind2, len(events)))
            if data.get("remove_nose"):
                batch = remove_event(batch, 0, 120, 990, 1050)
            filtered, _ = solv.preprocess(batch)
            est = solv.estimate(filtered, gt_flow, frame=im1, background=im0)
            roi = (slice(None), slice(common["xmin"], common["xmax"]), slice(common["ymin"], common["ymax"]))
            e0 = solv.calculate_flow_error(est[roi], gt_flow[roi])
            solv.save_flow_error_as_text(i_frame, e0, E.TEXT_WITHOUT_MASK)
            e1 = solv.calculate_flow_error(est[roi], gt_flow[roi], events=filtered, roi=common)
            solv.save_flow_error_as_text(i_frame, e1, E.TEXT_WITH_MASK)
            solv.save_flow_error_as_text(i_frame, {"t1": t1, "t2": t2}, E.TEXT_TIMESTAMPS)
            out["e0"].append(e0)
            out["e1"].append(e1)
            out["ts"].append({"t1": t1, "t2": t2})
            i_frame += 1
    return out


SMALL = ((128, 160), (0, 128, 16, 144))
WIDE = ((128, 1100), (0, 128, 960, 1088))      # wide enough for the driver's fixed remove_nose rectangle to bite
EVAL_CASES = {
    # name: (geometry, solver, frame method, filters, dt, remove_nose, n_events_per_batch, max_batch values)
    "pyramid_flow": (SMALL, "patch_eklt_pyramid2", "opencv_flow", None, 1, False, None, (1, 3, 16)),
    "pyramid_two_steps": (SMALL, "patch_eklt_pyramid2", "opencv_flow_two_steps", None, 2, False, 5000, (3,)),
    "dependent_flow": (SMALL, "patch_eklt_dependent", "opencv_flow", None, 1, False, None, (3,)),
    "pyramid_baf_hot": (SMALL, "patch_eklt_pyramid2", "opencv_flow", ["BAF", "HOT"], 1, False, None, (1, 3)),
    "no_prepared_path": (SMALL, "count", "opencv_flow", None, 1, False, None, (1, 3)),
    "pyramid_nose": (WIDE, "patch_eklt_pyramid2", "opencv_flow", None, 1, True, None, (16,)),
}
_LOOPS = {}


def _case(ebos, name, tmp_path_factory):
    """The recording, its config and the driver loop's results (computed once per case)."""
    if name not in _LOOPS:
        (shape, roi), method, flow, filters, dt, nose, n_events, _ = EVAL_CASES[name]
        tmp = tmp_path_factory.mktemp(name)
        events, frames, stamps = _recording(ebos, tmp / "rec", shape, 7, 6000 if shape[1] < 1000 else 30000)
        cfg = _config(shape, roi, method, 16, stamps, flow, filters, dt, nose, n_events)
        solv = _make_solver(ebos, copy.deepcopy(cfg), tmp / "loop")
        np.random.seed(21)
        want = _driver_loop(ebos, cfg, events, frames, solv)
        _LOOPS[name] = (events, frames, cfg, want, tmp)
    return _LOOPS[name]


def _same_dicts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in w:
            assert np.array_equal(np.float64(g[k]), np.float64(w[k]), equal_nan=True), (k, g[k], w[k])


@pytest.mark.parametrize("name,max_batch", [(n, mb) for n in sorted(EVAL_CASES) for mb in EVAL_CASES[n][7]])
def test_evaluator_equals_the_driver_loop(ebos, tmp_path_factory, name, max_batch):
    from event_based_bos_amd import evaluation as E

    events, frames, cfg, want, tmp = _case(ebos, name, tmp_path_factory)
    assert len(want["e0"]) >= 3
    out = tmp / f"eval_{max_batch}"
    solv = _make_solver(ebos, copy.deepcopy(cfg), out)
    np.random.seed(21)
    res = E.RecordingEvaluator(cfg, events, frames, solv).run(max_batch=max_batch)
    _same_dicts(res.errors_without_mask, want["e0"])
    _same_dicts(res.errors_with_mask, want["e1"])
    assert res.timestamps == want["ts"]
    assert [s.i_frame for s in res.steps] == list(range(len(want["ts"])))
    for fname in (E.TEXT_WITHOUT_MASK, E.TEXT_WITH_MASK, E.TEXT_TIMESTAMPS):
        assert open(out / fname).read() == open(tmp / "loop" / fname).read(), fname
    assert sorted(solv.evaluation_text_list) == sorted(str(out / f) for f in (E.TEXT_WITHOUT_MASK, E.TEXT_WITH_MASK))
    assert res.statistics["with_mask"]["EPE"]["n_data"] == len(want["e1"])
    if name == "pyramid_nose":
        assert cfg["data"]["remove_nose"] and all(np.isfinite(d["EPE"]) for d in res.errors_with_mask)


def test_evaluator_masked_epe_is_the_loops(ebos, tmp_path_factory):
    """The evaluator evaluates something real: its masked EPE of the pyramid solver is the driver loop's, a finite positive number."""
    from event_based_bos_amd import evaluation as E

    events, frames, cfg, want, tmp = _case(ebos, "pyramid_flow", tmp_path_factory)
    solv = _make_solver(ebos, copy.deepcopy(cfg), tmp / "sanity")
    np.random.seed(21)
    res = E.RecordingEvaluator(cfg, events, frames, solv).run(max_batch=4, poisson=True, keep_flows=True)
    got = np.array([d["EPE"] for d in res.errors_with_mask])
    assert np.array_equal(got, np.array([d["EPE"] for d in want["e1"]])) and np.all(np.isfinite(got)) and np.all(got > 0)
    H, W = cfg["data"]["height"], cfg["data"]["width"]
    assert len(res.flows) == len(res.poisson) == len(got)
    assert tuple(res.flows[0][0].shape) == (2, H, W) and tuple(res.poisson[0][0].shape) == (H, W) and res.flows[0][0].is_cuda
    assert all(b > 0 for b in res.batch_time_scales)


def test_evaluator_numbers_the_steps_around_a_skipped_frame(ebos, tmp_path_factory):
    """A directory of frame files one of which is narrower: the pairs that touch it are skipped, the others run, and the lines
    of the text files are numbered without a gap -- as the driver's loop numbers them.  ``save_dir`` goes before the
    visualizer's directory."""
    from PIL import Image

    from event_based_bos_amd import evaluation as E

    shape, roi = SMALL
    tmp = tmp_path_factory.mktemp("odd_frame")
    ev_path, fr_path, tr_path, stamps = E.synthetic_recording(str(tmp / "rec"), shape, 7, 6000, seed=6)
    stack = np.load(fr_path)
    os.makedirs(tmp / "frames")
    for i, f in enumerate(stack):
        Image.fromarray(f[:, :-20] if i == 3 else f).save(str(tmp / "frames" / f"{i:04d}.png"))
    events, frames = ebos.RawEventStore(ev_path), ebos.FrameStore(str(tmp / "frames"), tr_path)
    cfg = _config(shape, roi, "patch_eklt_pyramid2", 12, stamps)
    solv = _make_solver(ebos, copy.deepcopy(cfg), tmp / "loop")
    np.random.seed(4)
    want = _driver_loop(ebos, cfg, events, frames, solv)
    assert len(want["ts"]) == 2
    solv = _make_solver(ebos, copy.deepcopy(cfg), tmp / "viz")
    np.random.seed(4)
    res = E.RecordingEvaluator(cfg, events, frames, solv, save_dir=str(tmp / "eval")).run(max_batch=3)
    assert [(s.i1, s.i2) for s in res.skipped] == [(2, 3), (3, 4)] and [(s.i1, s.i2, s.i_frame) for s in res.steps] == [(1, 2, 0), (4, 5, 1)]
    _same_dicts(res.errors_with_mask, want["e1"])
    _same_dicts(res.errors_without_mask, want["e0"])
    for fname in (E.TEXT_WITHOUT_MASK, E.TEXT_WITH_MASK, E.TEXT_TIMESTAMPS):
        text = open(tmp / "eval" / fname).read()
        assert text == open(tmp / "loop" / fname).read(), fname
        assert [ln.split("::")[0] for ln in text.splitlines()] == ["frame 0", "frame 1"]
        assert not os.path.exists(tmp / "viz" / fname)
    assert sorted(solv.evaluation_text_list) == sorted(str(tmp / "eval" / f) for f in (E.TEXT_WITHOUT_MASK, E.TEXT_WITH_MASK))


def test_evaluator_skips_a_mis_sized_crop(ebos, tmp_path_factory):
    """crop_height / crop_width that the cropped frames do not have: every pair is skipped with a warning, nothing is written,
    i_frame does not advance -- as the driver's loop leaves it."""
    from event_based_bos_amd import evaluation as E

    events, frames, cfg, _, tmp = _case(ebos, "pyramid_flow", tmp_path_factory)
    bad = copy.deepcopy(cfg)
    bad["data"]["crop_width"] += 2
    solv = _make_solver(ebos, copy.deepcopy(cfg), tmp / "skipped_loop")
    want = _driver_loop(ebos, bad, events, frames, solv)
    assert want == {"e0": [], "e1": [], "ts": []}
    solv = _make_solver(ebos, copy.deepcopy(cfg), tmp / "skipped")
    res = E.RecordingEvaluator(bad, events, frames, solv).run(max_batch=3)
    assert res.steps == [] and res.errors_with_mask == [] and len(res.skipped) >= 3 and all(s.i_frame == 0 for s in res.skipped)
    assert not os.path.exists(tmp / "skipped" / E.TEXT_TIMESTAMPS)
