"""GPU checks of the frame warp (csrc/frame_warp.hip through ``event_based_bos_amd.frame_warp`` and ``FrameStore``) against the
numpy restatement tests/_warp_ref.py: bit for bit for uint8 frames and for INTER_NEAREST, within 8 * 2^-24 * max|src| for float32
INTER_LINEAR (four float32 products and three sums).  The restatement is held to the mathematics in tests/test_frame_warp.py; it
restates OpenCV's classic algorithm and is not checked against OpenCV."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _warp_ref as R  # noqa: E402
from _warp_cases import CASES, case_inputs  # noqa: E402

from event_based_bos_amd import FrameStore, frame_flow, frame_warp  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "golden_frame_warp.npz")
FARNEBACK = {"pyr_scale": 0.5, "levels": 4, "winsize": 10, "iterations": 3, "poly_n": 5, "poly_sigma": 1.2, "flags": 0}


def check(got: np.ndarray, want: np.ndarray, srcs: np.ndarray, flags: int, what: str):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    exact = srcs.dtype == np.uint8 or (flags & ~R.WARP_INVERSE_MAP) == R.INTER_NEAREST
    if exact:
        bad = int((got != want).sum())
        print(f"{what}: {bad} of {want.size} pixels differ")
        assert np.array_equal(got, want), what
    else:
        tol = 8 * 2.0 ** -24 * float(np.abs(srcs).max())
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print(f"{what}: max |difference| {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, what


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_restatement(name):
    srcs, M, dsize, flags, border, roi = case_inputs(name)
    want = R.warp_perspective_batch(srcs, M, dsize, flags, border, roi)
    got = frame_warp.warp_perspective_batch(srcs, M, dsize, flags, border, roi)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    check(got.cpu().numpy(), want, srcs, flags, name)
    one = frame_warp.warp_perspective(srcs[0], M if M.ndim == 2 else M[0], dsize, flags, border, roi)      # numpy in -> numpy out
    assert isinstance(one, np.ndarray)
    check(one, want[0], srcs, flags, name + " (single)")
    dev = frame_warp.warp_perspective(torch.from_numpy(srcs[0]).cuda(), M if M.ndim == 2 else M[0], dsize, flags, border, roi)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), one)


@pytest.mark.parametrize("name", ["rot_scale_u8", "rot_scale_f32", "full_roi_u8", "rot_scale_nearest_f32"])
def test_a_frame_alone_equals_the_frame_in_a_batch_of_8(name):
    srcs, M, dsize, flags, border, roi = case_inputs(name)
    rs = np.random.RandomState(5)
    others = rs.randint(0, 256, (7,) + srcs.shape[1:]).astype(np.uint8) if srcs.dtype == np.uint8 else \
        rs.uniform(-3, 3, (7,) + srcs.shape[1:]).astype(np.float32)
    alone = frame_warp.warp_perspective_batch(srcs[:1], M, dsize, flags, border, roi)
    for pos in (0, 3, 7):
        batch = np.concatenate([others[:pos], srcs[:1], others[pos:]])
        got = frame_warp.warp_perspective_batch(batch, M, dsize, flags, border, roi)
        assert got.shape[0] == 8 and torch.equal(got[pos], alone[0]), pos
    # ... and with one matrix per frame, the frame's own among eight different ones
    Ms = np.stack([np.asarray(M) @ np.array([[1, 0, 0.37 * k], [0, 1, -0.21 * k], [0, 0, 1.0]]) for k in range(8)]) \
        if not flags & R.WARP_INVERSE_MAP else None
    if Ms is not None:
        batch = np.concatenate([others[:2], srcs[:1], others[2:]])
        got = frame_warp.warp_perspective_batch(batch, Ms, dsize, flags, border, roi)
        assert torch.equal(got[2], frame_warp.warp_perspective_batch(srcs[:1], Ms[2], dsize, flags, border, roi)[0])


@pytest.mark.parametrize("name", ["full_u8", "full_f32", "per_frame_many_f32"])
def test_two_runs_are_bit_identical(name):
    srcs, M, dsize, flags, border, roi = case_inputs(name)
    dev = torch.from_numpy(srcs).cuda()
    a = frame_warp.warp_perspective_batch(dev, M, dsize, flags, border, roi)
    b = frame_warp.warp_perspective_batch(dev, M, dsize, flags, border, roi)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["rect_u8", "rot_scale_f32", "full_roi_u8"])
def test_rectangle_written_into_a_strided_view_equals_the_crop_of_the_full_output(name):
    srcs, M, dsize, flags, border, roi = case_inputs(name)
    W, H = dsize
    roi = roi or (5, H - 8, 6, W - 3)
    full = frame_warp.warp_perspective_batch(srcs, M, dsize, flags, border)
    crop = full[:, roi[0]:roi[1], roi[2]:roi[3]]
    assert torch.equal(frame_warp.warp_perspective_batch(srcs, M, dsize, flags, border, roi), crop)
    h, w, B = roi[1] - roi[0], roi[3] - roi[2], srcs.shape[0]
    for top, left, pad in ((0, 0, 0), (2, 3, 5), (1, 4, 8), (3, 1, 2)):            # aligned and unaligned row starts and strides
        canvas = torch.full((B, h + top + 2, w + left + pad), 99, dtype=full.dtype, device=full.device)
        view = canvas[:, top:top + h, left:left + w]
        got = frame_warp.warp_perspective_batch(srcs, M, dsize, flags, border, roi, out=view)
        assert got.data_ptr() == view.data_ptr() and torch.equal(view, crop), (top, left, pad)
        outside = canvas.clone()
        outside[:, top:top + h, left:left + w] = 99
        assert (outside == 99).all(), "wrote outside the view"


def test_strided_sources_are_read_in_place():
    srcs, M, dsize, flags, border, roi = case_inputs("rot_scale_u8")
    canvas = torch.zeros((3, 100, 150), dtype=torch.uint8, device="cuda")
    canvas[1, 4:94, 7:137] = torch.from_numpy(srcs[0]).cuda()
    view = canvas[1:2, 4:94, 7:137]
    want = frame_warp.warp_perspective_batch(srcs, M, dsize, flags, border)
    assert torch.equal(frame_warp.warp_perspective_batch(view, M, dsize, flags, border), want)


def _store(g, tmp_path, homography=True):
    trig = tmp_path / "trigger_events.txt"
    trig.write_text(str(g["trigger_text_old"]))
    return FrameStore(g["frames"], str(trig), g["homography"] if homography else None, tuple(int(v) for v in g["sensor_size"]))


def test_frame_store_load_images_equals_load_image_and_the_fixture(tmp_path):
    g = np.load(GOLDEN)
    store = _store(g, tmp_path)
    idx = [int(i) for i in g["load_indices"]]
    for k, i in enumerate(idx):
        image, t = store.load_image(i)
        assert isinstance(image, np.ndarray) and np.array_equal(image, g["warped_images"][k]) and t == g["load_timestamps"][k]
    batch, ts = store.load_images(idx)
    assert batch.is_cuda and np.array_equal(batch.cpu().numpy(), g["warped_images"]) and np.array_equal(ts, g["load_timestamps"])
    roi = {"xmin": 4, "xmax": 60, "ymin": 8, "ymax": 88}
    for pinned in (False, True):
        if pinned:
            store.pin()
        everything, ts = store.load_images(range(store.num_images), roi=roi)
        assert everything.shape == (store.num_images, 56, 80) and np.array_equal(ts, store.timestamps)
        for i in range(store.num_images):
            assert np.array_equal(everything[i].cpu().numpy(), frame_warp.validate_image(store.load_image(i)[0], roi))
        picked, _ = store.load_images([4, 1], roi=(4, 60, 8, 88))
        assert torch.equal(picked, everything[[4, 1]])
    with pytest.raises(AssertionError, match="odd number"):
        store.load_images([0], roi=(4, 59, 8, 88))
    raw, _ = _store(g, tmp_path, homography=False).load_images([0, 2], roi=(1, 95, 2, 126))
    assert np.array_equal(raw.cpu().numpy(), g["frames"][[0, 2], 1:95, 2:126])


def test_load_images_feeds_farneback_in_place(tmp_path):
    """End to end: the batch ``load_images(..., roi=common_params)`` returns, passed straight to ``farneback_batch``, gives the flow
    of the host-warped, host-cropped frames of the reference's path."""
    g = np.load(GOLDEN)
    store = _store(g, tmp_path)
    common = {"xmin": 4, "xmax": 60, "ymin": 8, "ymax": 88}
    frames, _ = store.load_images(range(4), roi=common)
    flow = frame_flow.farneback_batch(frames[:-1], frames[1:], FARNEBACK)
    host = np.stack([frame_warp.validate_image(store.load_image(i)[0], common) for i in range(4)])
    want = frame_flow.farneback_batch(host[:-1], host[1:], FARNEBACK)
    assert flow.shape == (3, 2, 56, 80) and torch.equal(flow, want) and float(flow.abs().max()) > 0
    # the crop as a view of the full warped frames is read in place as well
    full, _ = store.load_images(range(4))
    view = frame_warp.validate_image(full, common)                  # (a [4, H, W] batch: cropped along its last two axes)
    assert torch.equal(frame_warp.validate_image(full[:3], common), frames[:3])
    assert torch.equal(frame_flow.farneback_batch(view[:-1], view[1:], FARNEBACK), want)


def test_library_rejects_a_singular_matrix_and_unknown_flags():
    from event_based_bos_amd import _hip

    lib = _hip.require_gpu()
    src = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    m = np.zeros(9)
    args = (0, 1, 8, 8, src.data_ptr(), 64, 8, m.ctypes.data, 0, 8, 8)
    assert lib.ebos_warp_perspective(*args, 1, 0.0, 0, 8, 0, 8, out.data_ptr(), 64, 8, None) == -1
    assert lib.ebos_warp_perspective(*args, 4, 0.0, 0, 8, 0, 8, out.data_ptr(), 64, 8, None) == -3
