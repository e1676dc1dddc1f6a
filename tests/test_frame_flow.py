"""CPU checks of the frame-based flow (event_based_bos_amd/frame_flow.py, csrc/farneback.hip): the numpy restatement of
cv2.calcOpticalFlowFarneback the GPU tests hold the kernels against -- pinned on the reference's own wrapper
(tests/golden/golden_farneback.npz) and on the maths (an exact quadratic, a known sub-pixel shift) --, the public names, the C ABI
entries and the validation that needs no GPU."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import _farneback_ref as R
from _farneback_cases import CASES, YAML, case_config, case_frames, crop, stored_rows
from _poisson_ref import restated_image, restated_poisson

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_farneback.npz")
HEADER = os.path.join(ROOT, "include", "ebos_hip.h")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def restated_flow(a, b, params):
    """bos_optical_flow(a, b, params).transpose(2, 0, 1) with the restatement."""
    p = [params[k] for k in ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags")]
    return R.calc_optical_flow_farneback(a, b, None, *p).transpose(2, 0, 1)


def restated_padded(a, b, params):
    f = restated_flow(a, b, params)
    return np.pad(f, ((0, 0), (params["pad_x0"], params["pad_x1"]), (params["pad_y0"], params["pad_y1"])))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture(golden, name):
    c = CASES[name]
    f0, f1, f2 = case_frames(name)
    np.testing.assert_array_equal(golden[name + "_frames_sum"], [f.astype(np.float64).sum() for f in (f0, f1, f2)])
    params = case_config(name)["params_opencv_flow"]
    a0, a1, a2 = (crop(f, c["roi"]) for f in (f0, f1, f2))
    if c["method"] == "opencv_flow":
        got = restated_padded(a1, a2, params)
    else:
        p01, p02 = golden[name + "_p01"], golden[name + "_p02"]
        got = restated_flow(p01, p02, params)          # the second stage on the reference's pictures
        for f, p in ((restated_padded(a0, a1, params), p01), (restated_padded(a0, a2, params), p02)):
            img = restated_image(restated_poisson(f[1], f[0], np.zeros_like(f[0])))
            assert img.shape == p.shape and (np.abs(img.astype(int) - p.astype(int)) <= 1).all()
            assert (img != p).mean() < 1e-3
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got[:, stored_rows(name)], golden[name + "_flow"])
    assert np.abs(got).max() == golden[name + "_absmax"]


def test_fixture_covers_the_issue_cases(golden):
    assert int(golden["shimmed"]) == 1
    assert os.path.getsize(GOLDEN) < 512 * 1024
    dtypes = {CASES[n]["dtype"] for n in CASES}
    assert dtypes == {np.uint8, np.float32, np.float64}
    assert {CASES[n]["method"] for n in CASES} == {"opencv_flow", "opencv_flow_two_steps"}
    assert any(CASES[n]["roi"] is not None for n in CASES)
    shapes = {CASES[n]["shape"] for n in CASES}
    assert {(65, 87), (260, 346)} <= shapes
    ps = [CASES[n]["params"] for n in CASES]
    assert any(p["pyr_scale"] == 0.8 for p in ps) and any(p["poly_n"] == 7 and p["poly_sigma"] == 1.5 for p in ps)
    assert any(p["winsize"] % 2 == 1 for p in ps) and any(p["winsize"] == 1 for p in ps) and any(p["iterations"] == 1 for p in ps)
    # levels cut by the 32-pixel rule: the 80 x 96 ROI has one level below the frame with the YAML's 4
    assert len(R.level_plan(80, 96, 0.5, 4)) == 2
    # half-even rounding: 346 * 0.25 = 86.5 -> 86
    assert [(h, w) for _, _, h, w, _, _ in R.level_plan(260, 346, 0.5, 4)] == [(32, 43), (65, 86), (130, 173), (260, 346)]
    for n in CASES:
        if CASES[n]["roi"] is not None:
            x0, x1, y0, y1 = CASES[n]["roi"]
            H, W = CASES[n]["shape"]
            flow = golden[n + "_flow"]
            assert flow.shape[1:] == (H, W)
            if CASES[n]["method"] == "opencv_flow":       # zero outside the ROI
                assert not flow[:, :x0].any() and not flow[:, x1:].any() and not flow[:, :, :y0].any() and not flow[:, :, y1:].any()
                assert np.abs(flow[:, x0:x1, y0:y1]).max() > 0.5


def test_poly_exp_recovers_a_quadratic():
    """R = (b_row, b_col, A_rowrow, A_colcol, 2 A_rowcol) of f = c + b^T p + p^T A p around each interior pixel."""
    H, W = 40, 50
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    c, by, bx, ayy, axx, axy = 3.0, 0.7, -0.4, 0.02, -0.03, 0.015
    img = (c + by * y + bx * x + ayy * y * y + axx * x * x + axy * x * y).astype(np.float32)
    for n, sigma in ((5, 1.1), (5, 1.2), (7, 1.5)):
        Rr = R.poly_exp(img, n, sigma)
        inner = (slice(n, H - n), slice(n, W - n))
        yy, xx = y[inner], x[inner]
        want = [by + 2 * ayy * yy + axy * xx, bx + 2 * axx * xx + axy * yy, ayy + 0 * yy, axx + 0 * yy, axy + 0 * yy]
        for ch in range(5):
            np.testing.assert_allclose(Rr[ch][inner], want[ch], atol=1e-5 * max(1.0, np.abs(want[ch]).max()), err_msg=f"{n} {ch}")


def _smooth_texture(seed, H, W, dy, dx):
    rng = np.random.default_rng(seed)
    k = rng.uniform(-0.2, 0.2, (16, 2))
    ph = rng.uniform(0, 2 * np.pi, 16)
    a = rng.uniform(30, 60, 16)     # (OpenCV's 1e-3 regulariser of the 2 x 2 solve assumes a textured, high-contrast image)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return sum(a[i] * np.cos(k[i, 0] * (y - dy) + k[i, 1] * (x - dx) + ph[i]) for i in range(16)) + 128


@pytest.mark.parametrize("shift", [(0.31, -0.47), (-0.6, 0.22)])
def test_restatement_recovers_a_subpixel_shift(shift):
    """next(y, x) = prev(y - dy, x - dx): the flow at the centre is (dx, dy) (OpenCV's prev(y, x) ~ next(y + dy, x + dx))."""
    dy, dx = shift
    prev = _smooth_texture(0, 96, 128, 0, 0).astype(np.float32)
    nxt = _smooth_texture(0, 96, 128, dy, dx).astype(np.float32)
    f = R.calc_optical_flow_farneback(prev, nxt, None, 0.5, 3, 15, 3, 5, 1.2, 0)
    assert f.shape == (96, 128, 2) and f.dtype == np.float32
    c = f[46:50, 62:66].reshape(-1, 2)
    assert np.abs(c - [dx, dy]).max() < 0.02, c.mean(0)


def test_public_names_and_signatures(golden):
    import event_based_bos_amd as ebos
    from event_based_bos_amd import frame_flow as ff

    assert ebos.utils.bos_optical_flow is ff.bos_optical_flow and ebos.utils.pad_to_same_resolution is ff.pad_to_same_resolution
    ref = json.loads(str(golden["signatures"]))
    ours = {"FrameFlowEstimator.estimate": ff.FrameFlowEstimator.estimate,
            "FrameFlowEstimator.opencv_farneback": ff.FrameFlowEstimator.opencv_farneback,
            "FrameFlowEstimator.opencv_farneback_two_step": ff.FrameFlowEstimator.opencv_farneback_two_step,
            "FrameFlowEstimator.__init__": ff.FrameFlowEstimator.__init__,
            "bos_optical_flow": ff.bos_optical_flow, "pad_to_same_resolution": ff.pad_to_same_resolution}
    for k, f in ours.items():
        assert list(inspect.signature(f).parameters) == ref[k], k
    assert inspect.signature(ff.FrameFlowEstimator.opencv_farneback).parameters["visualize_frame"].default is False
    assert inspect.signature(ff.pad_to_same_resolution).parameters["constant_value"].default == 0.0
    assert list(inspect.signature(ff.calc_optical_flow_farneback).parameters) == [
        "prev", "next", "pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags"]
    assert list(inspect.signature(ff.farneback_batch).parameters) == ["prev", "next", "params"]


def test_pad_to_same_resolution_is_the_reference_rule():
    from event_based_bos_amd.utils import pad_to_same_resolution

    cfg = {"pad_x0": 1, "pad_x1": 2, "pad_y0": 3, "pad_y1": 0}
    a = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    got = pad_to_same_resolution(a, cfg, 0)
    assert got.shape == (2, 6, 7) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:, 1:4, 3:], a)
    assert got.sum() == a.sum()
    t = pad_to_same_resolution(torch.from_numpy(a), cfg, -1.0)
    assert tuple(t.shape) == (2, 6, 7) and float(t[0, 0, 0]) == -1.0


def test_header_entries_and_ctypes_table():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import SOURCES

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("ebos_farneback_scratch_bytes", "ebos_farneback"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_hip.SIGNATURES[name][1]), name
    assert "EBOS_FARNEBACK_U8 = 0" in text and "EBOS_FARNEBACK_F32 = 1" in text and "EBOS_FARNEBACK_F64 = 2" in text
    assert (_hip.FARNEBACK_U8, _hip.FARNEBACK_F32, _hip.FARNEBACK_F64) == (0, 1, 2)
    assert "farneback.hip" in SOURCES


def test_product_does_not_import_the_restatement():
    src = open(os.path.join(ROOT, "event_based_bos_amd", "frame_flow.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(_farneback_ref|oracle|cv2|tests)\b", src, flags=re.M)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    from event_based_bos_amd import _hip, frame_flow as ff

    def no_gpu(*a, **k):
        raise AssertionError("device work before validation")

    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    monkeypatch.setattr(ff, "default_device", no_gpu)
    f = np.zeros((40, 48), dtype=np.uint8)
    good = (0.5, 3, 15, 3, 5, 1.2)
    bad_params = [(1.0, 3, 15, 3, 5, 1.2), (0.0, 3, 15, 3, 5, 1.2), (0.5, -1, 15, 3, 5, 1.2), (0.5, 3, 0, 3, 5, 1.2),
                  (0.5, 3, 15, 0, 5, 1.2), (0.5, 3, 15, 3, 6, 1.2), (0.5, 3, 15, 3, 3, 1.2)]
    for p in bad_params:
        with pytest.raises(ValueError):
            ff.calc_optical_flow_farneback(f, f, *p)
    for flags in (4, 256):     # OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_FARNEBACK_GAUSSIAN
        with pytest.raises(NotImplementedError):
            ff.calc_optical_flow_farneback(f, f, *good, flags)
    with pytest.raises(ValueError):
        ff.calc_optical_flow_farneback(f, f[:, :40], *good)                      # shapes differ
    with pytest.raises(ValueError):
        ff.calc_optical_flow_farneback(f[None], f[None], *good)                  # not 2-D
    with pytest.raises(ValueError):
        ff.calc_optical_flow_farneback(f.astype(np.int16), f.astype(np.int16), *good)
    with pytest.raises(ValueError):
        ff.calc_optical_flow_farneback(f, f.astype(np.float32), *good)           # dtypes differ
    with pytest.raises(ValueError):
        ff.calc_optical_flow_farneback([[0, 1]], f, *good)
    with pytest.raises(ValueError):
        ff.farneback_batch(np.zeros((2, 40, 48), np.uint8), np.zeros((3, 40, 48), np.uint8), YAML)   # prev batch
    with pytest.raises(ValueError):
        ff.farneback_batch(f, f, YAML)                                           # not [B, H, W]
    with pytest.raises(ValueError):
        ff.farneback_batch(f[None], f[None], {"pyr_scale": 0.5})                 # missing params
    with pytest.raises(ValueError):
        ff.bos_optical_flow(f, f, dict(YAML, poly_n=9))
    est = ff.FrameFlowEstimator()
    cfg = {"params_opencv_flow": dict(YAML, pad_x0=0, pad_x1=0, pad_y0=0, pad_y1=0)}
    with pytest.raises(NotImplementedError, match="openpiv"):
        est.estimate("openpiv", f, f, f, cfg)
    with pytest.raises(NotImplementedError):
        est.estimate("rife", f, f, f, cfg)
    with pytest.raises(ValueError):
        est.estimate("opencv_flow_two_steps", f, f, f[:, :40], cfg)
    with pytest.raises(ValueError):
        est.estimate("opencv_flow", f, f, f, {"params_opencv_flow": dict(YAML, pad_x0=-1, pad_x1=0, pad_y0=0, pad_y1=0)})


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_without_a_gpu_the_product_raises():
    from event_based_bos_amd import HipUnavailableError, frame_flow as ff

    f = np.zeros((40, 48), dtype=np.uint8)
    with pytest.raises(HipUnavailableError):
        ff.calc_optical_flow_farneback(f, f, 0.5, 3, 15, 3, 5, 1.2)
    with pytest.raises(HipUnavailableError):
        ff.farneback_batch(f[None], f[None], YAML)
    with pytest.raises(HipUnavailableError):
        ff.FrameFlowEstimator().estimate("opencv_flow", f, f, f, {"params_opencv_flow": dict(YAML, pad_x0=0, pad_x1=0, pad_y0=0,
                                                                                              pad_y1=0)})
