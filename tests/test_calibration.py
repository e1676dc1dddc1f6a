"""CPU checks of the lens calibration (``event_based_bos_amd.calibration``): argument validation, the numpy restatement
tests/_rectify_ref.py held to the mathematics (the forward model undoes the inverse iteration), the host forward model against that
restatement, and the restatement's ``undistort_events`` against a fixture made by the reference's own function
(tests/golden/make_golden_rectify.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _rectify_ref as R  # noqa: E402

from event_based_bos_amd import CameraCalibration, FrameStore, RawEventStore, calibration, frame_warp, utils  # noqa: E402

def calib_of(name, **kw):
    return CameraCalibration(R.case_K(name), R.CASES[name]["D"], R.CASES[name]["size"], **kw)


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("n", [0, 1, 3, 6, 7, 9, 12, 14])
def test_length_of_D(n):
    with pytest.raises(ValueError, match="4, 5 or 8"):
        CameraCalibration(R.case_K("A"), np.zeros(n), (37, 70))


@pytest.mark.parametrize("n", [4, 5, 8])
def test_accepted_lengths_of_D(n):
    c = CameraCalibration(R.case_K("A"), np.arange(1, n + 1) * 1e-3, (37, 70))
    assert c.coefficients.shape == (8,) and np.array_equal(c.coefficients[:n], np.arange(1, n + 1) * 1e-3) and not c.coefficients[n:].any()


def test_bad_K_and_iterations_and_size():
    K = R.case_K("A")
    for bad in (np.diag([0.0, 57.0, 1.0]), np.diag([60.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="not invertible"):
            CameraCalibration(bad, np.zeros(5), (37, 70))
    with pytest.raises(ValueError, match="not invertible"):
        CameraCalibration(K, np.zeros(5), (37, 70), new_K=np.diag([0.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="3 x 3"):
        CameraCalibration(K[:2], np.zeros(5), (37, 70))
    with pytest.raises(ValueError, match="finite"):
        CameraCalibration(K * np.nan, np.zeros(5), (37, 70))
    skew = K.copy()
    skew[0, 1] = 0.1
    with pytest.raises(ValueError, match="skew"):
        CameraCalibration(skew, np.zeros(5), (37, 70))
    for it in (0, -1, 2.5, "a"):
        with pytest.raises(ValueError, match="iterations"):
            CameraCalibration(K, np.zeros(5), (37, 70), iterations=it)
    for size in ((0, 70), (37,), None, (37, 40000)):
        with pytest.raises(ValueError, match="sensor_size"):
            CameraCalibration(K, np.zeros(5), size)
    with pytest.raises(ValueError, match="finite"):
        CameraCalibration(K, [0, np.inf, 0, 0], (37, 70))


def test_shape_of_the_maps_in_undistort_events():
    ev = np.zeros((3, 4))
    m = np.zeros((5, 6))
    with pytest.raises(ValueError, match="one shape"):
        utils.undistort_events(ev, m, np.zeros((6, 5)), 5, 6)
    with pytest.raises(ValueError, match="2-D"):
        utils.undistort_events(ev, m.reshape(-1), m, 5, 6)
    with pytest.raises(ValueError, match="2-D"):
        utils.undistort_events(ev, m, np.zeros((0, 6)), 5, 6)
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        utils.undistort_events(np.zeros((3, 3)), m, m, 5, 6)
    with pytest.raises(ValueError, match="h and w"):
        utils.undistort_events(ev, m, m, -1, 6)


def test_validation_of_rectify_events_raw_and_undistort_image():
    c = calib_of("A")
    col = torch.zeros(4, dtype=torch.int16)
    t, p = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="float64 or torch.float32"):
        calibration.rectify_events_raw(col, col, t, p, c, dtype=torch.float16)
    with pytest.raises(ValueError, match="int16"):
        calibration.rectify_events_raw(col.int(), col, t, p, c)
    with pytest.raises(ValueError, match="equal length"):
        calibration.rectify_events_raw(col[:3], col, t, p, c)
    with pytest.raises(ValueError, match="CameraCalibration"):
        calibration.rectify_events_raw(col, col, t, p, {"K": None})
    with pytest.raises(ValueError, match="sensor"):
        frame_warp.undistort_image(np.zeros((40, 70), np.uint8), c)
    with pytest.raises(ValueError, match="uint8 or float32"):
        frame_warp.undistort_image(np.zeros((37, 70), np.float64), c)
    with pytest.raises(ValueError, match="singular"):
        frame_warp.undistort_image(np.zeros((37, 70), np.uint8), c, homography=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="roi"):
        frame_warp.undistort_image(np.zeros((37, 70), np.uint8), c, roi=(0, 38, 0, 70))


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_forward_model_undoes_the_inverse_iteration(name):
    K, D, size = R.case_K(name), R.CASES[name]["D"], R.CASES[name]["size"]
    grid = R.pixel_grid(*size)
    rmap = R.rectify_map(K, D, size)
    err = float(np.abs(R.distort_points(K, D, rmap) - grid).max())
    shift = float(np.sqrt(((rmap - grid) ** 2).sum(-1)).max())
    leaves = float((~((rmap[..., 0] >= 0) & (rmap[..., 0] < size[0]) & (rmap[..., 1] >= 0) & (rmap[..., 1] < size[1]))).mean())
    print(f"case {name}: round trip {err:.2e} px, largest shift {shift:.2f} px, {100 * leaves:.1f} % of pixels leave the image")
    assert err <= 1e-9
    if name == "A":
        assert 0.08 < leaves < 0.16 and 3.0 < shift < 7.0        # barrel: pixels move outwards, some beyond the image
    else:
        assert leaves == 0.0                                      # pincushion: no pixel leaves


def test_a_new_camera_matrix_is_applied_to_the_rectified_side_only():
    K, D, size = R.case_K("B"), R.CASES["B"]["D"], R.CASES["B"]["size"]
    nK = np.array([[70.0, 0, 50.0], [0, 75.0, 30.0], [0, 0, 1]])
    rmap = R.rectify_map(K, D, size, nK)
    assert np.abs(R.distort_points(K, D, rmap, nK) - R.pixel_grid(*size)).max() <= 1e-9
    base = R.rectify_map(K, D, size)
    want = np.stack([(base[..., 0] - K[1, 2]) / K[1, 1] * nK[1, 1] + nK[1, 2], (base[..., 1] - K[0, 2]) / K[0, 0] * nK[0, 0] + nK[0, 2]], -1)
    assert np.abs(rmap - want).max() <= 1e-11


@pytest.mark.parametrize("name", list(R.CASES))
def test_distort_points_is_the_restatement(name):
    K, D, size = R.case_K(name), R.CASES[name]["D"], R.CASES[name]["size"]
    nK = np.array([[K[0, 0] * 0.9, 0, K[0, 2] + 1.5], [0, K[1, 1] * 1.1, K[1, 2] - 0.5], [0, 0, 1]])
    pts = np.random.RandomState(3).uniform(-3, max(size) + 3, (5, 40, 2))
    for new_K in (None, nK):
        c = CameraCalibration(K, D, size, new_K=new_K)
        got = c.distort_points(pts)
        assert got.dtype == np.float64 and got.shape == pts.shape and np.array_equal(got, R.distort_points(K, D, pts, new_K))
    with pytest.raises(ValueError, match=r"\[\.\.\., 2\]"):
        c.distort_points(np.zeros((4, 3)))
    # the axes: a point on the optical axis stays; cx belongs to the column
    c = CameraCalibration(K, D, size)
    assert np.allclose(c.distort_points([K[1, 2], K[0, 2]]), [K[1, 2], K[0, 2]], atol=1e-12)


def test_from_dict_and_has_lens():
    assert CameraCalibration.from_dict({"K": None, "D": None}) is None
    assert CameraCalibration.from_dict({"K": R.case_K("A"), "D": None}, (37, 70)) is None
    assert CameraCalibration.from_dict({"K": None, "D": np.zeros(5)}, (37, 70)) is None
    c = CameraCalibration.from_dict({"K": R.case_K("A").tolist(), "D": list(R.CASES["A"]["D"])}, (37, 70))
    assert isinstance(c, CameraCalibration) and c.has_lens and c.iterations == 20 and np.array_equal(c.new_K, c.K)
    d = c.as_dict()
    assert set(d) == {"K", "D"} and np.array_equal(d["K"], R.case_K("A")) and np.array_equal(d["D"], R.CASES["A"]["D"])
    assert not CameraCalibration(R.case_K("A"), np.zeros(4), (37, 70)).has_lens
    assert CameraCalibration(R.case_K("A"), np.zeros(4), (37, 70), new_K=R.case_K("B")).has_lens
    cam = c.camera_array()
    assert cam.shape == (16,) and list(cam[:4]) == [60.0, 57.0, 34.8, 17.6] and list(cam[:4]) == list(cam[4:8])
    assert list(cam[8:13]) == list(R.CASES["A"]["D"]) and not cam[13:].any()


# ------------------------------------------------------------------ the stores
def columns(n=20, H=37, W=70, seed=0):
    rs = np.random.RandomState(seed)
    return {"x": rs.randint(0, W, n).astype(np.int16), "y": rs.randint(0, H, n).astype(np.int16),
            "t": np.sort(rs.randint(0, 50000, n)).astype(np.int32), "p": rs.randint(0, 2, n).astype(bool)}


def test_a_store_without_a_calibration_answers_as_the_reference():
    store = RawEventStore(columns())
    assert store.calibration is None and store.load_calib() == {"K": None, "D": None}
    with pytest.raises(NotImplementedError):
        store.undistort(store.load_event(0, 10))
    with pytest.raises(ValueError, match="calibration"):
        store.load_event(0, 10, rectify=True)
    with pytest.raises(ValueError, match="calibration"):
        store.plan(0, 10, (37, 70), rectify=True)
    assert np.array_equal(store.load_event(0, 10), store.load_event(0, 10, rectify=False))


def test_a_store_with_a_calibration():
    c = calib_of("A")
    store = RawEventStore(columns(), calibration=c)
    d = store.load_calib()
    assert np.array_equal(d["K"], c.K) and np.array_equal(d["D"], c.D)
    as_dict = RawEventStore(columns(), sensor_size=(37, 70), calibration={"K": c.K, "D": c.D})
    assert np.array_equal(as_dict.calibration.K, c.K) and as_dict.calibration.sensor_size == (37, 70)
    assert RawEventStore(columns(), calibration={"K": None, "D": None}).calibration is None
    with pytest.raises(ValueError, match="sensor_size"):
        RawEventStore(columns(), calibration={"K": c.K, "D": c.D})
    with pytest.raises(ValueError, match="calibration must be"):
        RawEventStore(columns(), calibration=3)
    for kw in ({"deferred": True}, {"emit": "compact"}):
        with pytest.raises(ValueError, match="integer-only"):
            store.plan(0, 10, (37, 70), rectify=True, **kw)
    with pytest.raises(ValueError, match="CameraCalibration"):
        FrameStore(np.zeros((1, 37, 70), np.uint8), np.array([10]), calibration={"K": c.K, "D": c.D})
    assert FrameStore(np.zeros((1, 37, 70), np.uint8), np.array([10]), calibration=c).calibration is c


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    from event_based_bos_amd import HipUnavailableError

    c = calib_of("A")
    with pytest.raises(HipUnavailableError):
        c.rectify_map()
    col = torch.zeros(4, dtype=torch.int16)
    with pytest.raises(HipUnavailableError):
        calibration.rectify_events_raw(col, col, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.bool), c)
    with pytest.raises(HipUnavailableError):
        utils.undistort_events(np.zeros((3, 4)), np.zeros((5, 6)), np.zeros((5, 6)), 5, 6)
    with pytest.raises(HipUnavailableError):
        utils.undistort_image(np.zeros((37, 70), np.uint8), c)
    with pytest.raises(HipUnavailableError):
        utils.undistort_image_batch(np.zeros((2, 37, 70), np.float32), c)
    store = RawEventStore(columns(), calibration=c)
    with pytest.raises(HipUnavailableError):
        store.undistort(store.load_event(0, 10))
    with pytest.raises(HipUnavailableError):
        store.load_event(0, 10, rectify=True)
    with pytest.raises(HipUnavailableError):
        FrameStore(np.zeros((1, 37, 70), np.uint8), np.array([10]), calibration=c).load_image(0)


# ------------------------------------------------------------------ the reference's undistort_events
@pytest.mark.parametrize("name", ["lens", "small"])
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_the_restatement_of_undistort_events_equals_the_reference(name, tag):
    ev, map_x, map_y, h, w, kept = R.golden_sets()[name]
    ev = ev.astype(np.float64 if tag == "f64" else np.float32)
    want = R.golden_output(ev, *kept[tag])
    got = R.undistort_events(ev, map_x, map_y, h, w)
    assert got.dtype == ev.dtype and np.array_equal(got, want)
    assert 0 < len(want) < len(ev)                                         # the maps send some events out
    neg = (ev[:, 0] < 0) | (ev[:, 1] < 0)
    assert neg.sum() > 10 and (ev[neg, :2] > -1).all()                     # negative fractional coordinates: pixel 0
    assert (ev[:, 0] != np.trunc(ev[:, 0])).sum() > 50                     # events off the grid


# ------------------------------------------------------------------ the ABI entries
def test_abi_symbols():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import PER_FILE_FLAGS, SOURCES

    assert "rectify.hip" in SOURCES and PER_FILE_FLAGS["rectify.hip"] == ["-ffp-contract=off"] and _hip.ABI_VERSION == 2
    names = ["ebos_rectify_map_f64", "ebos_rectify_scratch_bytes", "ebos_rectify_events_raw", "ebos_undistort_events_f32",
             "ebos_undistort_events_f64", "ebos_undistort_image_u8", "ebos_undistort_image_f32"]
    with open(os.path.join(os.path.dirname(HERE), "include", "ebos_hip.h")) as f:
        text = f.read()
    lib = _hip.load_library()
    for n in names:
        assert n in _hip.SIGNATURES and n + "(" in text and hasattr(lib, n)
    assert lib.ebos_rectify_scratch_bytes(1) > 0 and lib.ebos_rectify_scratch_bytes(10 ** 6) >= 4 * 10 ** 6
    # host-side validation comes before any launch: no GPU is needed to be refused
    cam = calib_of("A").camera_array()
    import ctypes as C

    INVALID_ARG = -1   # EBOS_ERR_INVALID_ARG
    assert lib.ebos_rectify_map_f64(cam.ctypes.data_as(C.c_void_p), 0, 37, 70, 16, None) == INVALID_ARG
    assert b"iterations" in lib.ebos_last_error()
    bad = cam.copy()
    bad[0] = 0.0
    assert lib.ebos_rectify_map_f64(bad.ctypes.data_as(C.c_void_p), 20, 37, 70, 16, None) == INVALID_ARG
    assert lib.ebos_rectify_events_raw(None, None, None, 0, None, -1, 1e6, 16, 37, 70, 37, 70, 0, None, 16, None, 0, None) \
        == INVALID_ARG
