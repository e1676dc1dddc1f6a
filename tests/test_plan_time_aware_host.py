"""Host-side checks of the time-aware recording path (no GPU needed): the argument errors of ``TimeAwarePlanStack.from_raw`` come
before the GPU is asked for, the host-only scratch query of ``ebos_plan_time_aware_raw_batch``, and the driver protocol --
``ContrastMaximization`` has ``estimate_batch_prepared``, so ``RecordingEvaluator`` takes its prepared path."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, TILE, T = 37, 70, (32, 32), 5


def _cols(n=100, t_dtype=torch.int32):
    return (torch.zeros(n, dtype=torch.int16), torch.zeros(n, dtype=torch.int16), torch.arange(n, dtype=t_dtype),
            torch.zeros(n, dtype=torch.uint8))


def _from_raw(cols=None, ranges=((0, 50), (25, 100)), image=(H, W), direction="first", tile=TILE, time_bin=T, **kw):
    from event_based_bos_amd import TimeAwarePlanStack

    return TimeAwarePlanStack.from_raw(_cols() if cols is None else cols, ranges, image, direction, tile, time_bin, **kw)


def test_from_raw_argument_errors_come_before_the_gpu():
    from event_based_bos_amd import EventPlan, _hip

    col, row, t, pol = _cols()
    with pytest.raises(ValueError, match="col"):
        _from_raw((col.to(torch.int32), row, t, pol))                        # dtype of a pixel column
    with pytest.raises(ValueError, match="row"):
        _from_raw((col, row.float(), t, pol))                                 # fractional coordinates keep the estimate_batch route
    with pytest.raises(ValueError, match="t must"):
        _from_raw((col, row, t.double(), pol))
    with pytest.raises(ValueError, match="1-D"):
        _from_raw((col[None], row, t, pol))                                   # shape
    with pytest.raises(ValueError, match="equal length"):
        _from_raw((col[:50], row, t, pol))
    with pytest.raises(ValueError, match="cols"):
        _from_raw((col, row))
    for bad in ((0, 101), (-1, 10), (60, 50)):
        with pytest.raises(IndexError, match="outside"):
            _from_raw(ranges=[(0, 50), bad])                                  # a range outside the columns
    with pytest.raises(ValueError, match="no windows"):
        _from_raw(ranges=[])
    with pytest.raises(ValueError, match="at most %d" % _hip.CMAX_VOXEL_MAX_BATCH):
        _from_raw(ranges=[(0, 1)] * (_hip.CMAX_VOXEL_MAX_BATCH + 1))
    for name, rect in (("roi", (10, 5, 0, 70)), ("roi", (0, 10, 70, 0)), ("remove", (10, 5, 0, 70)), ("roi", (0, 10, 0)),
                       ("remove", (0.5, 10, 0, 70))):
        with pytest.raises(ValueError, match=name):
            _from_raw(**{name: rect})                                         # a bad rectangle
    with pytest.raises(ValueError, match="tile"):
        _from_raw(tile=None)
    with pytest.raises(ValueError, match="tile"):
        _from_raw(tile="best")
    for bad_T in (0, 256):
        with pytest.raises(ValueError, match="time bins"):
            _from_raw(time_bin=bad_T)
    with pytest.raises(ValueError, match="direction"):
        _from_raw(direction="sideways")
    with pytest.raises(ValueError, match="image size"):
        _from_raw(image=(0, W))
    # the other name of the same build
    with pytest.raises(ValueError, match="tile"):
        EventPlan.build_raw_batch_time_aware(_cols(), [(0, 50)], (H, W), "first", None, T)
    # good arguments on host columns get as far as the device check
    with pytest.raises(_hip.HipUnavailableError):
        _from_raw(roi={"xmin": 0, "xmax": 30, "ymin": 5, "ymax": 60}, remove=(1, 2, 3, 4), cols=_cols(t_dtype=torch.int64))
    # the builds this one stands beside keep their refusals
    with pytest.raises(NotImplementedError):
        EventPlan.build_raw(*_cols(), (H, W), time_bin=T)


def test_scratch_query_is_host_only():
    """``ebos_plan_time_aware_batch_scratch_bytes``: 4 B of rank and a 16-byte record per event of the ranges, the scan's tile
    totals per window; never shrinking with the ranges; 0 for arguments the build refuses."""
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    lib = _hip.load_library()
    fn = lib.ebos_plan_time_aware_batch_scratch_bytes

    def ask(ranges, B=None, h=H, w=W, th=TILE[0], tw=TILE[1]):
        flat = [v for r in ranges for v in r]
        return int(fn((ctypes.c_int64 * len(flat))(*flat), len(ranges) if B is None else B, h, w, th, tw))

    prev = 0
    for n in (0, 1, 1000, 100_000, 3_000_000):
        got = ask([(0, n), (5, 5 + n)])
        assert got >= 2 * 20 * n and got >= prev and got <= 2 * 20 * n + (1 << 20), (n, got)
        prev = got
    assert ask([(0, 10)], h=720, w=1280, th=64, tw=64) > ask([(0, 10)])
    assert ask([(0, 10)], B=0) == 0 and ask([(0, 10)] * (_hip.CMAX_VOXEL_MAX_BATCH + 1)) == 0
    assert ask([(10, 5)]) == 0 and ask([(-1, 5)]) == 0 and ask([(0, 10)], h=0) == 0 and ask([(0, 10)], th=0) == 0
    assert ask([(0, 2 ** 31 - 1), (0, 1)]) == 0 and ask([(0, 2 ** 31 - 1)]) > 0
    assert int(fn(None, 1, H, W, *TILE)) == 0
    # and the entry point validates before any HIP call
    rc = lib.ebos_plan_time_aware_raw_batch(None, None, None, 0, 1e6, 0, (ctypes.c_int64 * 2)(0, 0), 1, *([0] * 10), 0, 0.0, 1, 0, H, W, *TILE,
                                            None, None, None, None, None, 0, None, None, 0, None, None, None, 0, None)
    assert rc == -1 and b"T = 0" in lib.ebos_last_error()


def _solver_config(native=True, **over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0, "tile": list(TILE),
           "patch": {"size": [12, 14], "sliding_window": [12, 14]},
           "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}},
           "time_aware": {"time_bin": T, "scheme": "upwind", "t0_location": "middle", "native": native}}
    cfg.update(over)
    return cfg


def test_contrast_maximization_takes_the_prepared_path():
    import event_based_bos_amd as ebos
    from event_based_bos_amd.evaluation import PreparedWindows, RecordingEvaluator

    make = ebos.solver.collections["contrast_maximization"]
    for cfg in (_solver_config(True), _solver_config(False), {"motion_model": "dense-flow"}):
        slv = make((H, W), (H, W), solver_config=cfg)
        assert callable(getattr(slv, "estimate_batch_prepared", None))
        assert slv._native_batch() == bool((cfg.get("time_aware") or {}).get("native", False))
        config = {"method": "opencv_flow", "estimation_method": "solver", "common_params": {"xmin": 0, "xmax": H, "ymin": 0, "ymax": W},
                  "data": {"height": H, "width": W}}
        assert RecordingEvaluator(config, None, None, slv).prepared_path is True
        # windows that do not carry their raw columns are refused before anything runs
        bare = PreparedWindows(torch.zeros(1, 2, H, W), torch.zeros(1, H, W), torch.zeros(1), torch.zeros(1), torch.ones(1))
        with pytest.raises(ValueError, match="raw columns"):
            slv.estimate_batch_prepared(bare)
        with pytest.raises(ValueError, match="max_batch"):
            slv.estimate_batch_prepared(PreparedWindows(None, None, None, torch.zeros(1), torch.ones(1), cols=_cols(), ranges=[(0, 5)]),
                                        max_batch=0)


def test_shipped_evaluation_config_selects_the_native_batch_family():
    """configs/cmax_time_aware_eval.yaml: the solver block builds a ``ContrastMaximization`` of the native batch family."""
    yaml = pytest.importorskip("yaml")
    import event_based_bos_amd as ebos

    with open(os.path.join(ROOT, "configs", "cmax_time_aware_eval.yaml")) as f:
        cfg = ebos.utils.propagate_config(yaml.safe_load(f))
    assert cfg["solver"]["method"] == "contrast_maximization" and cfg["solver"]["time_aware"]["native"] is True
    d = cfg["data"]
    slv = ebos.solver.collections[cfg["solver"]["method"]]((d["height"], d["width"]), (d["crop_height"], d["crop_width"]), {}, cfg["solver"])
    assert slv._native_batch() and hasattr(slv, "estimate_batch_prepared")
    assert slv.roi == tuple(cfg["common_params"][k] for k in ("xmin", "xmax", "ymin", "ymax"))
    assert np.isfinite(slv.lr) and slv.n_iter > 0
