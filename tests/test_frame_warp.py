"""CPU checks of the frame warp: the numpy restatement (tests/_warp_ref.py) held to the mathematics, the argument rules of
``event_based_bos_amd.frame_warp``, ``FrameStore`` against temporary files and against the fixture the reference's own
``CcsDataLoader`` produced (tests/golden/golden_frame_warp.npz), and the ABI entry.  Nothing here needs a GPU; what the kernel
computes is checked in tests/test_gpu_frame_warp.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _warp_ref as R  # noqa: E402
from _warp_cases import CASES, SMALL, case_inputs  # noqa: E402

from event_based_bos_amd import FrameStore, frame_warp  # noqa: E402
from event_based_bos_amd.data_loader import list_frame_files, read_trigger_timestamps  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "golden_frame_warp.npz")


def frame(seed, H=40, W=56, dtype=np.uint8):
    rs = np.random.RandomState(seed)
    f = rs.randint(0, 256, (H, W))
    return f.astype(np.uint8) if dtype == np.uint8 else (f / 16.0 - 3.0).astype(np.float32)


# ------------------------------------------------------------------ the restatement against the mathematics
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("flags", [R.INTER_LINEAR, R.INTER_NEAREST])
def test_identity_returns_the_source(dtype, flags):
    src = frame(1, dtype=dtype)
    out = R.warp_perspective(src, np.eye(3), (56, 40), flags)
    assert out.dtype == src.dtype and np.array_equal(out, src)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_integer_shift_moves_the_source_and_fills_the_border(dtype):
    src = frame(2, dtype=dtype)
    M = np.array([[1, 0, 3.0], [0, 1, -2.0], [0, 0, 1]])          # destination (x, y) = source (x - 3, y + 2)
    for flags in (R.INTER_LINEAR, R.INTER_NEAREST):
        out = R.warp_perspective(src, M, (56, 40), flags, border_value=7)
        want = np.full_like(src, 7)
        want[:38, 3:] = src[2:, :53]
        assert np.array_equal(out, want)


def test_half_pixel_shift_is_the_rounded_mean():
    src = frame(3)
    out = R.warp_perspective(src, np.array([[1, 0, -0.5], [0, 1, 0], [0, 0, 1]]), (55, 40))      # destination x samples source x + 1/2
    a, b = src[:, :-1].astype(int), src[:, 1:].astype(int)
    assert np.array_equal(out, ((a + b + 1) >> 1).astype(np.uint8))
    out = R.warp_perspective(src, np.array([[1, 0, 0], [0, 1, -0.5], [0, 0, 1]]), (56, 39))
    a, b = src[:-1].astype(int), src[1:].astype(int)
    assert np.array_equal(out, ((a + b + 1) >> 1).astype(np.uint8))


def test_table_is_the_closed_form_and_sums_to_one():
    """The kernel forms the weights as 32 (32 - fy | fy)(32 - fx | fx): exactly the restatement's table."""
    tab = R.interp_table()
    f = np.arange(32)
    lin = np.stack([32 - f, f], axis=1)
    assert np.array_equal(tab, 32 * lin[:, None, :, None] * lin[None, :, None, :])
    assert (tab.sum(axis=(2, 3)) == 32768).all() and tab.dtype == np.int32


def test_block_geometry():
    assert R.block_width(720, 1280) == 64 and R.block_width(9, 3) == 3 and R.block_width(8, 1000) == 128 and R.block_width(40, 56) == 56


@pytest.mark.parametrize("a,b,c", [(1, 1, 0), (-1, 1, 150), (1, -1, 100), (0, 2, 3)])
def test_ramp_is_reproduced_within_the_quantisation_bound(a, b, c):
    """On I = a x + b y + c every pixel whose four taps are inside differs from I at the exact coordinate by at most
    (|a| + |b|) / 64 (coordinates quantised to 1/32 px) + 0.5 (output rounding) + 4 * 255 * 2^-15 (weight rounding)."""
    Hs, Ws = 100, 140
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    ramp = a * xx + b * yy + c
    assert ramp.min() >= 0 and ramp.max() <= 255 and np.array_equal(ramp, np.rint(ramp))
    src = ramp.astype(np.uint8)
    M = np.array([[0.93, -0.11, 7.3], [0.08, 1.04, -3.9], [1.1e-4, -0.7e-4, 1.0]])
    W, H = 140, 100
    out = R.warp_perspective(src, M, (W, H), border_value=255)
    Mi = np.linalg.inv(M)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    w = Mi[2, 0] * x + Mi[2, 1] * y + Mi[2, 2]
    ex, ey = (Mi[0, 0] * x + Mi[0, 1] * y + Mi[0, 2]) / w, (Mi[1, 0] * x + Mi[1, 1] * y + Mi[1, 2]) / w
    X, Y = R.coordinates(R.invert3x3(M), (W, H), False)
    inside = ((X >> 5) >= 0) & ((X >> 5) + 1 < Ws) & ((Y >> 5) >= 0) & ((Y >> 5) + 1 < Hs)
    assert inside.sum() > 0.5 * H * W
    err = np.abs(out.astype(np.float64) - (a * ex + b * ey + c))[inside]
    bound = (abs(a) + abs(b)) / 64 + 0.5 + 4 * 255 * 2.0 ** -15
    print("max ramp error", err.max(), "bound", bound)
    assert err.max() <= bound


@pytest.mark.parametrize("name", ["rot_scale_u8", "rot_scale_f32", "rot_scale_nearest_u8", "small_homography_u8"])
def test_inverse_map_flag_with_the_inverse_equals_the_plain_call(name):
    srcs, M, dsize, flags, border, _ = case_inputs(name)
    plain = R.warp_perspective(srcs[0], M, dsize, flags, border)
    inv = R.warp_perspective(srcs[0], R.invert3x3(M), dsize, flags | R.WARP_INVERSE_MAP, border)
    assert np.array_equal(plain, inv)


@pytest.mark.parametrize("name", ["rot_scale_u8", "rot_scale_f32", "partly_outside_u8", "w_zero_line_u8", "rot_scale_nearest_f32"])
def test_a_pixel_does_not_depend_on_the_rectangle(name):
    srcs, M, dsize, flags, border, _ = case_inputs(name)
    full = R.warp_perspective(srcs[0], M, dsize, flags, border)
    H, W = full.shape
    for roi in ((0, H, 0, W), (3, H - 5, 7, W - 2), (5, 6, 1, 2), (H - 1, H, W - 3, W), (0, 17, W // 2 - 1, W // 2 + 2)):
        part = R.warp_perspective(srcs[0], M, dsize, flags, border, roi)
        assert np.array_equal(part, full[roi[0]:roi[1], roi[2]:roi[3]]), roi


def test_w_zero_line_and_outside_pixels_take_the_border():
    srcs, M, dsize, flags, border, _ = case_inputs("w_zero_line_u8")
    out = R.warp_perspective(srcs[0], M, dsize, flags, border)
    X, Y = R.coordinates(M, dsize, False)
    assert (X[5] == 0).all() and (Y[5] == 0).all()                # W == 0: the scale is 0, the coordinate (0, 0) with no fraction
    assert (out[5] == srcs[0][0, 0]).all() and (out[:5] == 33).mean() > 0.5
    srcs, M, dsize, flags, border, _ = case_inputs("partly_outside_u8")
    out = R.warp_perspective(srcs[0], M, dsize, flags, border)
    assert 0.05 < (out == 200).mean() < 0.95


def test_every_case_is_well_formed():
    for name in CASES:
        c = CASES[name]
        M = np.asarray(c["M"])
        assert M.shape[-2:] == (3, 3) and (M.ndim == 2 or M.shape[0] == c.get("frames", 1))
    for name in SMALL:
        srcs, M, dsize, flags, border, roi = case_inputs(name)
        out = R.warp_perspective_batch(srcs, M, dsize, flags, border, roi)
        assert out.dtype == srcs.dtype and out.shape[0] == srcs.shape[0]
        if "nan_coordinate" in name:
            assert (out == R.border_as(out.dtype, border)).all()      # every coordinate clamps to INT_MAX: outside the source
        elif "identity" not in name:
            assert out.std() > 0


# ------------------------------------------------------------------ the package's argument rules (raised before any GPU work)
def test_argument_errors_come_before_any_library_call(monkeypatch):
    from event_based_bos_amd import _hip

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_hip, "require_gpu", boom)
    monkeypatch.setattr(frame_warp, "default_device", boom)
    src, eye = frame(4), np.eye(3)
    wp, wb = frame_warp.warp_perspective, frame_warp.warp_perspective_batch
    with pytest.raises(ValueError, match="2 dimensions"):
        wp(src[None], eye, (56, 40))
    with pytest.raises(ValueError, match="3 dimensions"):
        wb(src, eye, (56, 40))
    with pytest.raises(ValueError, match="uint8 or float32"):
        wp(src.astype(np.float64), eye, (56, 40))
    with pytest.raises(ValueError, match="uint8 or float32"):
        wp(torch.zeros(4, 5, dtype=torch.int16), eye, (5, 4))
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        wp([[1, 2], [3, 4]], eye, (2, 2))
    with pytest.raises(ValueError, match="3 x 3"):
        wp(src, np.eye(4), (56, 40))
    with pytest.raises(ValueError, match="3 x 3"):
        wb(src[None].repeat(3, 0), np.stack([eye] * 2), (56, 40))
    with pytest.raises(ValueError, match="not finite"):
        wp(src, np.array([[1, 0, np.nan], [0, 1, 0], [0, 0, 1]]), (56, 40))
    with pytest.raises(ValueError, match="not finite"):
        wp(src, np.array([[1, 0, np.inf], [0, 1, 0], [0, 0, 1]]), (56, 40), frame_warp.WARP_INVERSE_MAP | 1)
    with pytest.raises(ValueError, match="singular"):
        wp(src, np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]]), (56, 40))
    with pytest.raises(ValueError, match=r"M\[1\] is singular"):
        wb(src[None].repeat(2, 0), np.stack([eye, np.zeros((3, 3))]), (56, 40))
    for flags in (2, 3, 4, 7, 8, 17 + 1, 32, -1, 1.5, None, "linear"):
        with pytest.raises(NotImplementedError, match="INTER_NEAREST.*INTER_LINEAR.*WARP_INVERSE_MAP"):
            wp(src, eye, (56, 40), flags)
    for dsize in ((0, 40), (56,), (56.5, 40), None, (56, 70000)):
        with pytest.raises(ValueError, match="dsize"):
            wp(src, eye, dsize)
    for roi in ((0, 41, 0, 56), (-1, 40, 0, 56), (5, 5, 0, 56), (0, 40, 10, 57), (0, 40, 0), {"xmin": 0, "xmax": 40, "ymin": 0}):
        with pytest.raises(ValueError, match="roi"):
            wp(src, eye, (56, 40), roi=roi)
    with pytest.raises(ValueError, match="border_value"):
        wp(src, eye, (56, 40), border_value=np.nan)
    with pytest.raises(ValueError, match="out must be"):
        wb(src[None], eye, (56, 40), out=torch.zeros(1, 40, 56, dtype=torch.uint8))
    # a singular matrix is the caller's to pass with WARP_INVERSE_MAP (it is then not inverted): that passes validation
    with pytest.raises(AssertionError, match="the library was reached"):
        wp(src, np.zeros((3, 3)), (56, 40), frame_warp.WARP_INVERSE_MAP | frame_warp.INTER_LINEAR)


def test_constants_and_exports():
    import event_based_bos_amd as ebos

    assert (frame_warp.INTER_NEAREST, frame_warp.INTER_LINEAR, frame_warp.WARP_INVERSE_MAP) == (0, 1, 16)
    assert ebos.warp_perspective is frame_warp.warp_perspective and ebos.warp_perspective_batch is frame_warp.warp_perspective_batch
    assert ebos.validate_image is frame_warp.validate_image and ebos.FrameStore is FrameStore and ebos.frame_warp is frame_warp


def test_validate_image_is_the_drivers_crop():
    cfg = {"xmin": 2, "xmax": 30, "ymin": 4, "ymax": 44}
    img = frame(5)
    assert np.array_equal(frame_warp.validate_image(img, cfg), img[2:30, 4:44])
    t = torch.from_numpy(img)
    assert torch.equal(frame_warp.validate_image(t, cfg), t[2:30, 4:44])
    with pytest.raises(AssertionError, match="29 rows, an odd number"):
        frame_warp.validate_image(img, dict(cfg, xmax=31))
    with pytest.raises(AssertionError, match="41 columns, an odd number"):
        frame_warp.validate_image(img, dict(cfg, ymax=45))
    # a batch is cropped along its last two axes and judged by them: nine frames are as good as eight
    batch = np.stack([img] * 9)
    assert np.array_equal(frame_warp.validate_image(batch, cfg), batch[:, 2:30, 4:44])
    assert torch.equal(frame_warp.validate_image(torch.from_numpy(batch), cfg), torch.from_numpy(batch)[:, 2:30, 4:44])
    with pytest.raises(AssertionError, match="odd number"):
        frame_warp.validate_image(batch[:8], dict(cfg, ymax=45))
    with pytest.raises(AssertionError, match="odd number"):
        frame_warp.validate_image(batch[:8, :, :], dict(cfg, xmin=3))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    from event_based_bos_amd import HipUnavailableError

    with pytest.raises(HipUnavailableError):
        frame_warp.warp_perspective(frame(6), np.eye(3), (56, 40))
    store = FrameStore(frame(7)[None], np.array([10]), np.eye(3), (40, 56))
    with pytest.raises(HipUnavailableError):
        store.load_image(0)
    with pytest.raises(HipUnavailableError):
        store.load_images([0])


# ------------------------------------------------------------------ the ABI entry
def test_abi_symbol_and_host_side_validation():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import SOURCES, build_library

    assert "frame_warp.hip" in SOURCES and "ebos_warp_perspective" in _hip.SIGNATURES
    build_library(verbose=False)
    lib = _hip.load_library()
    assert lib.ebos_version() == _hip.ABI_VERSION == 2
    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    sing = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)
    p = C.c_void_p(16)        # never dereferenced: every call below is rejected before a launch

    def call(dtype=0, B=1, Hs=8, Ws=8, m=eye, ms=0, H=8, W=8, flags=1, border=0.0, rect=(0, 8, 0, 8), src=p, out=p, osr=8):
        return lib.ebos_warp_perspective(dtype, B, Hs, Ws, src, 64, 8, C.cast(m, C.c_void_p), ms, H, W, flags, border, *rect, out, 64, osr, None)

    assert call(dtype=2) == -1 and b"dtype" in lib.ebos_last_error()
    assert call(B=0) == -1 and call(Hs=0) == -1 and call(W=0) == -1 and call(Hs=40000) == -1
    assert call(src=None) == -1 and call(out=None) == -1
    assert call(ms=5) == -1 and b"stride" in lib.ebos_last_error()
    assert call(rect=(0, 9, 0, 8)) == -1 and b"rectangle" in lib.ebos_last_error()
    assert call(rect=(0, 8, 4, 4)) == -1 and call(osr=4) == -1
    assert call(border=float("nan")) == -1
    assert call(flags=2) == -3 and b"INTER_NEAREST" in lib.ebos_last_error()
    assert call(flags=1 | 32) == -3
    assert call(m=sing) == -1 and b"singular" in lib.ebos_last_error()


# ------------------------------------------------------------------ FrameStore
OLD_FORMAT = "1000 0 1\n1500 0 0\n2000 0 1\n2500 0 0\n4000 0 1\n"
NEW_FORMAT = "1,0,1000\n0,0,1500\n1,0,2000\n0,0,2500\n1,0,4000\n"


@pytest.mark.parametrize("text", [OLD_FORMAT, NEW_FORMAT])
def test_both_timestamp_formats_keep_positive_edges(tmp_path, text):
    path = tmp_path / "trigger_events.txt"
    path.write_text(text)
    assert np.array_equal(read_trigger_timestamps(str(path)), [1000, 2000, 4000])
    store = FrameStore(np.zeros((3, 4, 6), np.uint8), str(path))
    assert np.array_equal(store.timestamps, np.array([1000, 2000, 4000]) / 1e6) and store.num_images == 3


def test_timestamp_arrays():
    old = np.array([[1000, 0, 1], [1500, 0, 0], [2000, 0, 1]])
    assert np.array_equal(read_trigger_timestamps(old), [1000, 2000])
    assert np.array_equal(read_trigger_timestamps(old[:, ::-1], "new"), [1000, 2000])
    assert np.array_equal(read_trigger_timestamps(np.array([5, 9])), [5, 9])
    with pytest.raises(ValueError):
        read_trigger_timestamps(np.zeros((3, 2), int))
    with pytest.raises(ValueError):
        read_trigger_timestamps(np.array([0.5, 1.0]))
    with pytest.raises(ValueError):
        read_trigger_timestamps(old, "other")


def test_time_to_image_index_is_searchsorted_minus_one():
    store = FrameStore(np.zeros((4, 4, 6), np.uint8), np.array([1_000_000, 2_000_000, 2_500_000, 4_000_000]))
    assert [store.time_to_image_index(t) for t in (0.5, 1.0, 1.0000001, 1.7, 2.0, 2.5, 3.9, 4.0, 9.0)] == [-1, -1, 0, 0, 0, 1, 2, 2, 3]
    assert store.image_index_to_time(2) == 2.5 and store.image_index_to_time(-1) == 4.0


def test_load_image_without_a_homography_is_the_raw_frame(tmp_path):
    stack = np.stack([frame(10 + k) for k in range(3)])
    ts = np.array([10, 20, 30])
    for source in (stack, str(tmp_path / "frames.npy"), str(tmp_path / "frames.npz"), str(tmp_path / "only.npz")):
        if isinstance(source, str) and source.endswith("frames.npy"):
            np.save(source, stack)
        elif isinstance(source, str) and source.endswith("frames.npz"):
            np.savez(source, frames=stack, other=np.zeros(3))
        elif isinstance(source, str):
            np.savez(source, stack)
        store = FrameStore(source, ts)
        assert store.num_images == 3 and not store.warp_frame
        for k in range(3):
            image, t = store.load_image(k)
            assert np.array_equal(image, stack[k]) and image.dtype == np.uint8 and t == ts[k] / 1e6
    with pytest.raises(IndexError):
        store.load_image(3)


def test_directory_of_image_files(tmp_path):
    from PIL import Image

    stack = np.stack([frame(20 + k, 12, 18) for k in range(3)])
    d = tmp_path / "frames"
    d.mkdir()
    for k in (2, 0, 1):
        Image.fromarray(stack[k]).save(str(d / f"frame_{k:04d}.png"))
    (d / "notes.txt").write_text("not an image")
    (d / "README").write_text("no suffix")
    (d / "FRAME_9999.PNG.bak").write_text("a backup")
    assert [os.path.basename(f) for f in list_frame_files(str(d))] == ["frame_0000.png", "frame_0001.png", "frame_0002.png"]
    store = FrameStore(str(d), np.array([1, 2, 3]))
    assert store.num_images == 3
    for k in range(3):
        assert np.array_equal(store.load_image(k)[0], stack[k])


def test_frame_store_argument_errors(tmp_path):
    stack, ts = np.zeros((2, 4, 6), np.uint8), np.array([1, 2])
    with pytest.raises(ValueError, match="N, Hs, Ws"):
        FrameStore(stack[0], ts)
    with pytest.raises(ValueError, match="uint8 or float32"):
        FrameStore(stack.astype(np.int32), ts)
    with pytest.raises(ValueError, match="3 x 3"):
        FrameStore(stack, ts, np.eye(2), (4, 6))
    with pytest.raises(ValueError, match="sensor_size"):
        FrameStore(stack, ts, np.eye(3))
    with pytest.raises(ValueError, match="neither"):
        FrameStore(str(tmp_path / "frames.mp4"), ts)
    with pytest.raises(ValueError):
        FrameStore(12, ts)
    store = FrameStore(stack, ts, np.eye(3), (4, 6))
    with pytest.raises(IndexError):
        store.load_images([0, 2])
    with pytest.raises(ValueError, match="no frame"):
        store.load_images([])
    with pytest.raises(ValueError, match="roi"):
        store.load_images([0], roi=(0, 5, 0, 6))
    with pytest.raises(AssertionError, match="3 rows, an odd number"):        # as validate_image would refuse it
        store.load_images([0], roi=(0, 3, 0, 6))
    with pytest.raises(AssertionError, match="5 columns, an odd number"):
        store.load_images([0], roi=(0, 4, 1, 6))
    with pytest.raises(IndexError):                                            # stricter than the reference: -1 is not the last frame
        store.load_image(-1)


def test_frame_store_against_the_reference_loader_fixture(tmp_path):
    """golden_frame_warp.npz: the reference's own CcsDataLoader on a synthetic sequence (cv2 shimmed: the fixture pins the
    wrapper -- dsize order, loadtxt of the homography, positive edges, the index arithmetic -- not OpenCV's bits)."""
    g = np.load(GOLDEN)
    assert int(g["shimmed"]) == 1
    frames = g["frames"]
    for fmt in ("old", "new"):
        trig, hom = tmp_path / f"trigger_{fmt}.txt", tmp_path / "homography.txt"
        trig.write_text(str(g["trigger_text_" + fmt]))
        hom.write_text(str(g["homography_text"]))
        store = FrameStore(frames, str(trig), str(hom), tuple(int(v) for v in g["sensor_size"]))
        assert store.num_images == int(g["num_images"])
        assert np.array_equal(store.timestamps, g["timestamps_" + fmt])
        assert np.array_equal(store.homography, g["homography"])
        idx = g["image_index_to_time_in"]
        assert np.array_equal([store.image_index_to_time(int(i)) for i in idx], g["image_index_to_time_out_" + fmt])
        assert [store.time_to_image_index(float(t)) for t in g["time_to_image_index_in"]] == list(g["time_to_image_index_out_" + fmt])
    # the reference without data.warp: the raw frame
    plain = FrameStore(frames, str(trig))
    for k, i in enumerate(g["load_indices"]):
        image, t = plain.load_image(int(i))
        assert np.array_equal(image, g["raw_images"][k]) and t == g["load_timestamps"][k]
    # ... and with it: what the reference handed cv2.warpPerspective, and what came back, is the restatement on the same call
    W, H = (int(v) for v in g["warp_dsize"])
    assert (H, W) == tuple(int(v) for v in g["sensor_size"])
    for k, i in enumerate(g["load_indices"]):
        assert np.array_equal(R.warp_perspective(frames[int(i)], g["homography"], (W, H)), g["warped_images"][k])
