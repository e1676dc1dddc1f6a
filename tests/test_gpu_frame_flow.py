"""GPU checks of the frame-based flow (event_based_bos_amd/frame_flow.py, csrc/farneback.hip): every case of
tests/golden/golden_farneback.npz through FrameFlowEstimator, the YAML geometry against the numpy restatement, a BOS-style
random-dot physics check, batching and determinism, strided views and the driver's protocol."""
import json
import os

import numpy as np
import pytest
import torch

import _farneback_ref as R
from _farneback_cases import CASES, YAML, case_config, case_frames, crop, stored_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_farneback.npz")
DEV = torch.device("cuda")
# observed on an MI355X and set about 10x above: the kernels repeat the restatement's float32 operations, so only
# the order of the float64 window sums differs
REL_L2 = 1e-4
MAX_ABS = 1e-2


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _ff():
    from event_based_bos_amd import frame_flow
    return frame_flow


def errors(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = got - want
    return float(np.linalg.norm(d) / max(np.linalg.norm(want), 1e-30)), float(np.abs(d).max())


def assert_close(got, want, what, max_abs=MAX_ABS):
    rel, mx = errors(got, want)
    print(f"{what}: rel-L2 {rel:.3e} max|d| {mx:.3e}")
    assert rel <= REL_L2 and mx <= max_abs, (what, rel, mx)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases(golden, name):
    ff = _ff()
    c = CASES[name]
    f0, f1, f2 = case_frames(name)
    cfg = case_config(name)
    params = cfg["params_opencv_flow"]
    flow = ff.FrameFlowEstimator().estimate(c["method"], crop(f0, c["roi"]), crop(f1, c["roi"]), crop(f2, c["roi"]), cfg)
    assert isinstance(flow, np.ndarray) and flow.dtype == np.float32 and flow.shape == (2,) + c["shape"]
    want = golden[name + "_flow"]
    bar = MAX_ABS if params["winsize"] > 1 else 1e-4 * float(golden[name + "_absmax"])
    if c["method"] == "opencv_flow":
        assert_close(flow[:, stored_rows(name)], want, name, bar)
        return
    p01, p02 = golden[name + "_p01"], golden[name + "_p02"]
    second = ff.farneback_batch(p01[None], p02[None], params)[0].cpu().numpy()      # the second stage on the stored pictures
    assert_close(second[:, stored_rows(name)], want, name + " (second stage)", bar)
    # the whole chain: the pictures may differ by one LSB where poisson_image documents it; the flow must then follow
    first = ff.farneback_batch(crop(f0, c["roi"])[None], np.stack([crop(f1, c["roi"]), crop(f2, c["roi"])]), params)
    H, W = c["shape"]
    full = torch.zeros((2, 2, H, W), device=DEV)
    full[:, :, params["pad_x0"]:H - params["pad_x1"], params["pad_y0"]:W - params["pad_y1"]] = first
    from event_based_bos_amd.poisson import poisson_image
    pics = poisson_image(full).cpu().numpy()
    diff = np.abs(pics.astype(int) - np.stack([p01, p02]).astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3, name
    if not diff.any():
        assert_close(flow[:, stored_rows(name)], want, name + " (chain)", bar)


def test_yaml_geometry_against_the_restatement():
    """720 x 640 (the YAML's ROI crop) with the YAML's params, uint8."""
    ff = _ff()
    rng = np.random.default_rng(11)
    H, W = 720, 640
    base = rng.integers(0, 256, size=(H // 4 + 2, W // 4 + 2)).astype(np.float32)
    big = np.kron(base, np.ones((4, 4), np.float32))
    prev = R.gaussian_blur(big, 9, 2.0)[:H, :W].astype(np.uint8)
    nxt = R.gaussian_blur(big, 9, 2.0)[1:H + 1, 2:W + 2].astype(np.uint8)
    got = ff.calc_optical_flow_farneback(prev, nxt, *(YAML[k] for k in ff.PARAM_KEYS))
    want = R.calc_optical_flow_farneback(prev, nxt, None, *(YAML[k] for k in ff.PARAM_KEYS))
    assert got.shape == (H, W, 2) and got.dtype == np.float32
    assert_close(got, want, "720x640 YAML")
    assert abs(np.median(got[100:-100, 100:-100, 0]) + 2) < 0.1 and abs(np.median(got[100:-100, 100:-100, 1]) + 1) < 0.1


def _dots(H, W, seed, disp=None):
    """A BOS background: Gaussian dots (sigma 1.2 px) at random centres, moved by disp(y, x) -> (dy, dx); uint8."""
    rng = np.random.default_rng(seed)
    n = H * W // 12
    cy, cx = rng.uniform(-4, H + 4, n), rng.uniform(-4, W + 4, n)
    amp = rng.uniform(0.6, 1.0, n)
    if disp is not None:
        dy, dx = disp(cy, cx)
        cy, cx = cy + dy, cx + dx
    img = np.zeros((H, W))
    for oy in range(-4, 5):
        for ox in range(-4, 5):
            iy, ix = np.floor(cy).astype(int) + oy, np.floor(cx).astype(int) + ox
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            v = amp * np.exp(-((iy - cy) ** 2 + (ix - cx) ** 2) / (2 * 1.2 ** 2))
            np.add.at(img, (iy[ok], ix[ok]), v[ok])
    return np.clip(img * 160 + 20, 0, 255).astype(np.uint8)


def test_physics_random_dot_background():
    """Dots moved by a smooth bump (peak 2 px in x, 1 px in y): the GPU's median end-point error in the interior matches the
    restatement's within 1e-3 px and is small."""
    ff = _ff()
    H, W = 192, 256

    def bump(y, x):
        g = np.exp(-((y - H / 2) ** 2 + (x - W / 2) ** 2) / (2 * 40.0 ** 2))
        return 1.0 * g, 2.0 * g

    prev, nxt = _dots(H, W, 3), _dots(H, W, 3, bump)
    yy, xx = np.meshgrid(np.arange(H, dtype=float), np.arange(W, dtype=float), indexing="ij")
    gy, gx = bump(yy, xx)          # prev(y, x) ~ next(y + dy, x + dx)
    got = ff.calc_optical_flow_farneback(prev, nxt, *(YAML[k] for k in ff.PARAM_KEYS))
    want = R.calc_optical_flow_farneback(prev, nxt, None, *(YAML[k] for k in ff.PARAM_KEYS))
    inner = (slice(16, H - 16), slice(16, W - 16))
    epe = lambda f: float(np.median(np.hypot(f[..., 0][inner] - gx[inner], f[..., 1][inner] - gy[inner])))  # noqa: E731
    e_gpu, e_ref = epe(got), epe(want)
    print(f"median EPE: GPU {e_gpu:.4f} px, restatement {e_ref:.4f} px")
    assert abs(e_gpu - e_ref) <= 1e-3
    assert e_gpu <= 0.1


def test_batch_shared_prev_and_determinism():
    ff = _ff()
    f0, f1, f2 = case_frames("s260x346_u8")
    params = YAML
    t0, t1, t2 = (torch.from_numpy(f).to(DEV) for f in (f0, f1, f2))
    single = [ff.farneback_batch(t0[None], t[None], params) for t in (t1, t2)]
    pairs = ff.farneback_batch(torch.stack([t0, t0]), torch.stack([t1, t2]), params)
    shared = ff.farneback_batch(t0[None], torch.stack([t1, t2]), params)
    again = ff.farneback_batch(t0[None], torch.stack([t1, t2]), params)
    assert pairs.shape == (2, 2, 260, 346) and pairs.dtype == torch.float32 and pairs.is_cuda
    for b in range(2):
        assert torch.equal(pairs[b], single[b][0]) and torch.equal(shared[b], single[b][0])
    assert torch.equal(shared, again)
    one = ff.calc_optical_flow_farneback(t1, t2, *(params[k] for k in ff.PARAM_KEYS))
    assert one.is_cuda and one.shape == (260, 346, 2)
    assert torch.equal(one.permute(2, 0, 1), ff.farneback_batch(t1[None], t2[None], params)[0])


def test_strided_views_match_contiguous_copies():
    ff = _ff()
    f0, f1, f2 = case_frames("s260x346_u8")
    a, b = f1[10:250, 20:300], f2[10:250, 20:300]         # ROI views of larger frames
    assert not a.flags.c_contiguous
    want = ff.calc_optical_flow_farneback(np.ascontiguousarray(a), np.ascontiguousarray(b), *(YAML[k] for k in ff.PARAM_KEYS))
    np.testing.assert_array_equal(ff.calc_optical_flow_farneback(a, b, *(YAML[k] for k in ff.PARAM_KEYS)), want)
    ta, tb = torch.from_numpy(f1).to(DEV)[10:250, 20:300], torch.from_numpy(f2).to(DEV)[10:250, 20:300]
    got = ff.calc_optical_flow_farneback(ta, tb, *(YAML[k] for k in ff.PARAM_KEYS))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    f32 = torch.from_numpy(np.stack([f1, f2]).astype(np.float32)).to(DEV)[:, 10:250, 20:300]
    np.testing.assert_array_equal(ff.farneback_batch(f32[:1], f32[1:], YAML)[0].permute(1, 2, 0).cpu().numpy(), want)


def test_driver_protocol():
    """bos_event.py:136-155: validate_image crops of 720 x 1280 uint8 frames, estimate('opencv_flow') with the propagated YAML."""
    ff = _ff()
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_hot_plate1.json")))["propagated"]
    common = cfg["common_params"]
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(182, 322)).astype(np.float32)
    big = R.gaussian_blur(np.kron(base, np.ones((4, 4), np.float32)), 9, 2.0)
    ims = [big[i:i + 720, 2 * i:2 * i + 1280].astype(np.uint8) for i in range(3)]
    crops = [im[..., common["xmin"]:common["xmax"], common["ymin"]:common["ymax"]] for im in ims]
    flow = ff.FrameFlowEstimator().estimate(cfg["method"], crops[0], crops[1], crops[2], cfg)
    assert isinstance(flow, np.ndarray) and flow.dtype == np.float32 and flow.shape == (2, 720, 1280)
    roi = (slice(None), slice(common["xmin"], common["xmax"]), slice(common["ymin"], common["ymax"]))
    outside = np.ones(flow.shape, bool)
    outside[roi] = False
    assert not flow[outside].any()
    inside = ff.farneback_batch(np.ascontiguousarray(crops[1])[None], np.ascontiguousarray(crops[2])[None], cfg["params_opencv_flow"])
    np.testing.assert_array_equal(flow[roi], inside[0].cpu().numpy())
    assert abs(np.median(flow[roi][0][50:-50, 50:-50]) + 2) < 0.1 and abs(np.median(flow[roi][1][50:-50, 50:-50]) + 1) < 0.1
