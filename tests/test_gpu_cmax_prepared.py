"""GPU tests of ``ContrastMaximization.estimate_batch_prepared`` and of ``RecordingEvaluator`` driving a time-aware native solver
through it.

The prepared route builds the stacked time-aware plan of a batch from the raw sensor columns (``TimeAwarePlanStack.from_raw``); the
route it is compared with, ``estimate_batch`` on the windows' event arrays, builds the plans window by window.  The two hold the same
events and differ only in the order of the events of one source pixel, the difference tests/test_gpu_voxel_loop_batch.py's
``test_solver_estimate_batch`` bounds: its bars are used here unchanged (per-iteration loss deviation <= BATCH_LOOP_FACTOR x the largest
measured deviation of the single loop on that kind of window; flow and patch-flow relative L2 < 1e-3)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxel_loop_cases as C  # noqa: E402
from _voxel_loop_cases import H, N, T5, W, rel  # noqa: E402
from test_gpu_voxel_loop_batch import BATCH_LOOP_FACTOR, SINGLE_LOOP_DEVIATION  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3
TPS = 1e6


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def tolerance(b):
    return BATCH_LOOP_FACTOR * max(SINGLE_LOOP_DEVIATION[f"w{b}"])


def prepared_windows(ebos, seed=61):
    """Three windows of integer-pixel events as raw columns of one store, the kinds of ``test_solver_estimate_batch``: w0 20 000 events,
    w1 its first, every third interior and last event, w2 = w0 plus 3 000 events on one pixel with times all over the window."""
    def make():
        from event_based_bos_amd.evaluation import window_ingest_raw_batch

        rs = np.random.RandomState(seed)
        row, col = rs.randint(0, H, N).astype(np.int16), rs.randint(0, W, N).astype(np.int16)
        ticks = np.sort(rs.randint(0, 10_000, N)).astype(np.int64)
        pol = rs.randint(0, 2, N).astype(np.uint8)
        pick = np.concatenate([[0], np.arange(1, N - 1)[::3], [N - 1]])
        hot_t = rs.randint(int(ticks[0]) + 1, int(ticks[-1]), C.HOT_EXTRA)
        order = np.argsort(np.concatenate([ticks, hot_t]), kind="stable")
        w2 = [np.concatenate([a, b])[order] for a, b in ((col, np.full(C.HOT_EXTRA, C.HOT_PIXEL[1], np.int16)),
                                                         (row, np.full(C.HOT_EXTRA, C.HOT_PIXEL[0], np.int16)), (ticks, hot_t),
                                                         (pol, rs.randint(0, 2, C.HOT_EXTRA).astype(np.uint8)))]
        windows = [(col, row, ticks, pol), (col[pick], row[pick], ticks[pick], pol[pick]), tuple(w2)]
        cols = [np.concatenate([w[k] + (20_000 * i if k == 2 else 0) for i, w in enumerate(windows)]) for k in range(4)]
        cols[2] = cols[2].astype(np.int32)
        bounds = np.concatenate([[0], np.cumsum([len(w[0]) for w in windows])])
        ranges = [(int(bounds[i]), int(bounds[i + 1])) for i in range(B)]
        dev_cols = tuple(torch.from_numpy(np.ascontiguousarray(c)).to(C.dev()) for c in cols)
        return window_ingest_raw_batch(dev_cols, ranges, (H, W), None, None, TPS)
    return C.cached(("prepared_windows", seed), make)


# ---------------------------------------------------------------------------------------------- 6. the native family
@pytest.mark.parametrize("pyramid", [False, True])
def test_prepared_route_follows_estimate_batch(ebos, pyramid):
    prepared = prepared_windows(ebos)
    assert [int(c) for c in prepared.count.cpu()] == [N, len(range(1, N - 1)[::3]) + 2, N + C.HOT_EXTRA]
    windows = [prepared.events(b).cpu().numpy() for b in range(B)]
    cfg = C.solver_config(True, n_iter=5)
    if pyramid:                                                   # two scales, and patches with too few events are not estimated
        cfg["patch"] = {"pyramid": {"coarsest": 16, "finest": 8}, "do_event_thresholding": True, "event_thres": 120}
    make = ebos.solver.collections["contrast_maximization"]

    def solver():
        slv = make((H, W), (H, W), solver_config=cfg)
        if not pyramid:
            slv.previous_best = C.theta_start() * 0.2             # the warm start is every window's start
        return slv

    ref = solver()
    want = ref.estimate_batch(windows, max_batch=8)
    want_hist, want_theta = [list(h) for h in ref.histories], [t.clone() for t in ref.patch_flows]
    n_scales = len(ref.pyramid_scales())
    for max_batch in (8, 2):
        slv = solver()
        flows = slv.estimate_batch_prepared(prepared, frames=None, background=None, max_batch=max_batch)
        assert isinstance(flows, np.ndarray) and flows.shape == (B, 2, H, W) and flows.dtype == np.float64 and np.isfinite(flows).all()
        assert slv.loop_modes == ["native-batch"] * n_scales and n_scales == (2 if pyramid else 1) and slv.loop_mode == "native-batch"
        assert len(slv.histories) == B and len(slv.patch_flows) == B and slv.history == slv.histories[-1]
        assert torch.equal(slv.patch_flow, slv.patch_flows[-1])
        for b in range(B):
            assert len(slv.histories[b]) == len(want_hist[b]) == sum(n for _, _, n in slv.pyramid_scales())
            dev = np.abs(np.array(slv.histories[b]) - np.array(want_hist[b])) / np.abs(np.array(want_hist[b]))
            r_flow, r_theta = rel(flows[b], want[b]), rel(slv.patch_flows[b], want_theta[b])
            print(f"pyramid={pyramid} max_batch={max_batch} window {b}: history deviation {dev.tolist()} (bar {tolerance(b):.3e}), "
                  f"flow rel L2 {r_flow:.3e}, patch-flow rel L2 {r_theta:.3e}")
            assert (dev <= tolerance(b)).all(), (b, dev, tolerance(b))
            assert r_flow < 1e-3 and r_theta < 1e-3, (b, r_flow, r_theta)
        if pyramid:                                               # the masks are each window's own
            plan = ebos.EventPlan.build(C.G(windows[1]), (H, W), "first", True, tile=C.TILE, emit="full", time_bin=T5)
            mask = slv.patch_mask(plan, (8, 8), (8, 8)).cpu().numpy()
            theta = slv.patch_flows[1].cpu().numpy()
            assert (mask == 0).any() and (mask == 1).any() and (theta[:, mask == 0] == 0).all() and (theta[:, mask == 1] != 0).any()
            full = slv.patch_mask(ebos.EventPlan.build(C.G(windows[0]), (H, W), "first", True, tile=C.TILE, emit="full", time_bin=T5),
                                  (8, 8), (8, 8)).cpu().numpy()
            assert not np.array_equal(full, mask)
        on_device = solver().estimate_batch_prepared(prepared, max_batch=max_batch, device_out=True)
        assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and on_device.dtype == torch.float64
        dev_rel = max(rel(on_device[b], flows[b]) for b in range(B))
        print(f"pyramid={pyramid} max_batch={max_batch}: device_out against the numpy result, largest rel L2 {dev_rel:.3e}")
        assert tuple(on_device.shape) == (B, 2, H, W) and dev_rel < 1e-3


# ---------------------------------------------------------------------------------------------- 7. outside the family
def test_outside_the_native_family_the_windows_are_estimated_one_by_one(ebos):
    """The default patch-flow Adam configuration (no ``time_aware`` block) on integer-pixel events: lean plans, whose loop gives the same
    bits on every call -- first checked, then used: the prepared route is ``estimate`` on the same float64 events."""
    prepared = prepared_windows(ebos)
    windows = [prepared.events(b).cpu().numpy() for b in range(B)]
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0, "tile": list(C.TILE),
           "patch": {"size": list(C.PATCH), "sliding_window": list(C.PATCH)},
           "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}}}
    make = ebos.solver.collections["contrast_maximization"]

    def solver():
        slv = make((H, W), (H, W), solver_config=cfg)
        slv.previous_best = C.theta_start() * 0.2
        return slv

    first, second = solver().estimate_batch(windows), solver().estimate_batch(windows)
    self_distance = max(rel(first[b], second[b]) for b in range(B))
    print(f"estimate_batch against itself: array_equal {np.array_equal(first, second)}, largest rel L2 {self_distance:.3e}")
    assert np.array_equal(first, second)
    slv = solver()
    assert not slv._native_batch()
    got = slv.estimate_batch_prepared(prepared, max_batch=2)
    print(f"estimate_batch_prepared against estimate_batch: largest rel L2 {max(rel(got[b], first[b]) for b in range(B)):.3e}")
    assert got.dtype == np.float64 and np.array_equal(got, first)
    assert len(slv.histories) == B and slv.history == slv.histories[-1] and slv.loop_mode != "native-batch"
    dev = solver().estimate_batch_prepared(prepared, device_out=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), first)


# ---------------------------------------------------------------------------------------------- 8. the evaluator
SHAPE, ROI = (64, 96), (0, 64, 16, 80)


class _Sequential(object):
    """The solver without its ``estimate_batch_prepared``: the evaluator drives it through ``preprocess`` + ``estimate``, window by
    window -- the route a time-aware solver took before it had the method."""

    def __init__(self, solver):
        object.__setattr__(self, "_solver", solver)

    def __getattr__(self, name):
        if name == "estimate_batch_prepared":
            raise AttributeError(name)
        return getattr(object.__getattribute__(self, "_solver"), name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, "_solver"), name, value)


def _eval_config(ebos, stamps, filters):
    solver = {"method": "contrast_maximization", "motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance",
              "outer_padding": 0, "patch": {"size": [16, 24], "sliding_window": [16, 24]},
              "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}},
              "time_aware": {"time_bin": T5, "scheme": "upwind", "t0_location": "middle", "native": True},
              "filter": {"filters": filters, "parameters": {"BAF_continuous_update": True, "BAF_dt": 0.005, "BAF_ksize": 1,
                                                             "BAF_num_support_event": 1, "HOT_thresh": 10}}}
    cfg = {"common_params": {"n_frames": 1, "xmin": ROI[0], "xmax": ROI[1], "ymin": ROI[2], "ymax": ROI[3]},
           "data": {"height": SHAPE[0], "width": SHAPE[1], "remove_nose": False},
           "estimation_method": "solver", "method": "opencv_flow",
           "evaluation": {"metrics": ["flow"], "time_list": [[float(stamps[0]) + 0.004, float(stamps[-1]) + 0.004]]},
           "params_opencv_flow": {"flags": 0, "iterations": 3, "levels": 3, "poly_n": 5, "poly_sigma": 1.2, "pyr_scale": 0.5, "winsize": 10},
           "solver": solver}
    return ebos.utils.propagate_config(cfg)


_RECORDINGS = {}


def _recording(ebos, tmp_path_factory):
    if "rec" not in _RECORDINGS:
        from event_based_bos_amd.evaluation import synthetic_recording

        tmp = tmp_path_factory.mktemp("cmax_prepared")
        ev_path, fr_path, tr_path, stamps = synthetic_recording(str(tmp / "rec"), SHAPE, 8, 4000, seed=5, hot_pixel=(SHAPE[0] // 2, SHAPE[1] - 40))
        _RECORDINGS["rec"] = (ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path), stamps, tmp)
    return _RECORDINGS["rec"]


@pytest.mark.parametrize("filters", [None, ["BAF", "HOT"]], ids=["crop", "baf_hot"])
def test_evaluator_drives_the_time_aware_solver_in_batches(ebos, tmp_path_factory, filters):
    from event_based_bos_amd import evaluation as E

    events, frames, stamps, tmp = _recording(ebos, tmp_path_factory)
    cfg = _eval_config(ebos, stamps, filters)
    d = cfg["data"]
    make = ebos.solver.collections["contrast_maximization"]
    tag = "crop" if filters is None else "baf_hot"

    def run(wrap, max_batch, name):
        slv = make((d["height"], d["width"]), (d["crop_height"], d["crop_width"]), {}, cfg["solver"], None)
        assert slv._native_batch()
        ev = E.RecordingEvaluator(cfg, events, frames, _Sequential(slv) if wrap else slv, save_dir=str(tmp / f"{tag}_{name}"))
        assert ev.prepared_path is (not wrap)
        res = ev.run(max_batch=max_batch)
        return res, slv, str(tmp / f"{tag}_{name}")

    want, seq_solver, want_dir = run(True, 3, "sequential")
    assert len(want.steps) >= 3 and seq_solver.loop_mode == "native"
    for max_batch in (1, 3):
        got, slv, got_dir = run(False, max_batch, f"prepared_{max_batch}")
        assert slv.loop_mode == "native-batch"
        assert [s.i_frame for s in got.steps] == [s.i_frame for s in want.steps] and got.timestamps == want.timestamps
        assert open(os.path.join(got_dir, E.TEXT_TIMESTAMPS)).read() == open(os.path.join(want_dir, E.TEXT_TIMESTAMPS)).read()
        assert got.batch_time_scales == want.batch_time_scales
        for kind, a, b in (("without mask", got.errors_without_mask, want.errors_without_mask),
                           ("with mask", got.errors_with_mask, want.errors_with_mask)):
            for key in ("EPE", "AE"):
                va, vb = np.array([e[key] for e in a]), np.array([e[key] for e in b])
                dev = np.abs(va - vb) / np.abs(vb)
                print(f"{tag} max_batch={max_batch} {kind} {key}: sequential {vb.tolist()}, prepared {va.tolist()}, relative {dev.tolist()}")
                assert np.isfinite(va).all() and np.isfinite(vb).all() and (vb > 0).all()
                assert (dev < 1e-3).all(), (kind, key, dev)
