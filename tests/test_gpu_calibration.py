"""GPU checks of the lens calibration (csrc/rectify.hip through ``event_based_bos_amd.calibration``, ``frame_warp.undistort_image``
and the two stores) against the numpy restatement tests/_rectify_ref.py, the host forward model and the fixture made by the
reference's ``undistort_events``.  OpenCV is absent where this package is developed: the image path is checked against the
restatement and the forward model, not against ``cv2.undistort``.

Bounds.  The map against the forward model: 1e-9 px (the restatement itself returns to the grid within 1.2e-13 px at 20
iterations; the margin covers any difference between division sequences).  The map against the restatement: 1e-12 px (bit-equality is
expected with contraction off, and printed).  Events, ``undistort_events`` and images: exact."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _rectify_ref as R  # noqa: E402
import _warp_ref as WR  # noqa: E402

from event_based_bos_amd import (CameraCalibration, EventPlan, FrameStore, RawEventStore, calibration, frame_warp,  # noqa: E402
                                 utils)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCAN_TILE = 4096          # keys per workgroup of the device-wide scan (event_plan.hip); its second level starts beyond 256 tiles
BLOCK = 256               # events per workgroup pass of the flag and scatter kernels


def calib_of(name, **kw):
    return CameraCalibration(R.case_K(name), R.CASES[name]["D"], R.CASES[name]["size"], **kw)


_MAPS = {}


def gpu_map(name) -> np.ndarray:
    """The GPU's map of a case, built once and shared (read-only)."""
    if name not in _MAPS:
        m = calib_of(name).rectify_map(DEV).cpu().numpy()
        m.setflags(write=False)
        _MAPS[name] = m
    return _MAPS[name]


# ------------------------------------------------------------------ the map
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_map_through_the_forward_model_is_the_pixel_grid(name):
    c = calib_of(name)
    m = gpu_map(name)
    assert m.shape == c.sensor_size + (2,) and m.dtype == np.float64
    err = float(np.abs(c.distort_points(m) - R.pixel_grid(*c.sensor_size)).max())
    print(f"case {name}: round trip {err:.3e} px")
    assert err <= 1e-9


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_map_equals_the_restatement(name):
    want = R.rectify_map(R.case_K(name), R.CASES[name]["D"], R.CASES[name]["size"])
    got = gpu_map(name)
    err = float(np.abs(got - want).max())
    print(f"case {name}: max |GPU - restatement| {err:.3e} px, bit-identical: {np.array_equal(got, want)}")
    assert err <= 1e-12


def test_the_map_with_a_new_camera_matrix_and_another_iteration_count():
    K, D, size = R.case_K("B"), R.CASES["B"]["D"], R.CASES["B"]["size"]
    nK = np.array([[70.0, 0, 50.0], [0, 75.0, 30.0], [0, 0, 1]])
    got = CameraCalibration(K, D, size, new_K=nK, iterations=7).rectify_map(DEV).cpu().numpy()
    assert np.abs(got - R.rectify_map(K, D, size, nK, 7)).max() <= 1e-12


def test_no_lens_gives_the_pixel_grid():
    c = CameraCalibration(R.case_K("A"), np.zeros(5), (37, 70))
    err = float(np.abs(c.rectify_map(DEV).cpu().numpy() - R.pixel_grid(37, 70)).max())
    print(f"D = 0: max distance from the grid {err:.3e} px")
    assert err <= 1e-12


def test_two_builds_are_bit_identical_and_the_map_is_cached():
    a, b = calib_of("A"), calib_of("A")
    ma = a.rectify_map(DEV)
    assert ma.is_cuda and ma.dtype == torch.float64 and a.rectify_map(DEV) is ma          # cached per device
    assert torch.equal(ma, b.rectify_map(DEV)) and np.array_equal(ma.cpu().numpy(), gpu_map("A"))


# ------------------------------------------------------------------ events
def raw_columns(n, name, seed=0, content="inside", t64=False, pol_bool=True):
    H, W = R.CASES[name]["size"]
    rs = np.random.RandomState(seed)
    col, row = rs.randint(0, W, n).astype(np.int16), rs.randint(0, H, n).astype(np.int16)
    if content == "corner":
        col[:], row[:] = 0, 0
    elif content == "outside":                       # a third each: col >= W, row >= H, negative
        k = np.arange(n) % 6
        col[k == 1], row[k == 2] = W, H
        col[k == 3], row[k == 4] = -1, -3
        col[k == 5] = 32767
    t = np.sort(rs.randint(0, 50000, n))
    t = (t + 2 ** 33).astype(np.int64) if t64 else t.astype(np.int32)
    p = rs.randint(0, 2, n)
    return col, row, t, (p.astype(bool) if pol_bool else (p * 3).astype(np.uint8))   # uint8: any non-zero value is "on"


def run_events(cols, calib, dtype=torch.float64):
    ev, n_sensor, n_image = calibration.rectify_events_raw(*(torch.from_numpy(c).to(DEV) for c in cols), calib, dtype=dtype)
    assert ev.is_cuda and ev.dtype == dtype and ev.ndim == 2 and ev.shape[1] == 4
    return ev.cpu().numpy(), n_sensor, n_image


def check_events(cols, name, dtype=torch.float64, what=""):
    want, ws, wi = R.rectify_events_raw(*cols, gpu_map(name), dtype=np.float64 if dtype == torch.float64 else np.float32)
    got, gs, gi = run_events(cols, calib_of(name), dtype)
    print(f"{what or name}: n = {len(cols[0])}, kept {len(got)} (restatement {len(want)}), outside the sensor {gs} ({ws}), outside the image {gi} ({wi})")
    assert got.shape == want.shape and (gs, gi) == (ws, wi) and np.array_equal(got, want)
    return got


@pytest.mark.parametrize("n", [0, 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17, SCAN_TILE, SCAN_TILE + 1, 3 * SCAN_TILE + 17,
                               256 * SCAN_TILE + SCAN_TILE + 5])
def test_events_equal_the_restatement_at_every_size(n):
    got = check_events(raw_columns(n, "A", seed=n % 97), "A")
    assert got.shape == ((0, 4) if n == 0 else got.shape) and (n < BLOCK or 0 < len(got) < n)


def test_every_event_kept():
    cols = raw_columns(3 * BLOCK + 17, "B", seed=1)
    got = check_events(cols, "B")
    assert len(got) == len(cols[0])
    # t and p are what load_event gives without a calibration, bit for bit
    plain = RawEventStore(dict(zip("xytp", cols))).load_event(0, len(cols[0]))
    assert np.array_equal(got[:, 2:], plain[:, 2:])
    assert (got[:, :2] != plain[:, :2]).any()


def test_every_event_dropped():
    m = gpu_map("A")[0, 0]
    assert m[0] < 0 or m[1] < 0, "the corner pixel of case A is expected to leave the image"
    cols = raw_columns(2 * BLOCK + 3, "A", content="corner")
    got, n_sensor, n_image = run_events(cols, calib_of("A"))
    assert got.shape == (0, 4) and n_sensor == 0 and n_image == len(cols[0])
    check_events(cols, "A")


@pytest.mark.parametrize("name", ["A", "B"])
def test_events_outside_the_sensor_are_dropped_and_counted(name):
    cols = raw_columns(5 * BLOCK + 1, name, seed=2, content="outside")
    H, W = R.CASES[name]["size"]
    got, n_sensor, _ = run_events(cols, calib_of(name))
    outside = (cols[0] < 0) | (cols[0] >= W) | (cols[1] < 0) | (cols[1] >= H)
    assert n_sensor == int(outside.sum()) > len(cols[0]) // 2
    check_events(cols, name)


@pytest.mark.parametrize("t64", [False, True])
@pytest.mark.parametrize("pol_bool", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_every_type_of_column_and_output(t64, pol_bool, dtype):
    cols = raw_columns(SCAN_TILE + 99, "A", seed=3, t64=t64, pol_bool=pol_bool)
    got = check_events(cols, "A", dtype, what=f"t64={t64} bool={pol_bool} {dtype}")
    # t and p against load_event of an uncalibrated store on the same columns (the kept rows, cast to the output type)
    plain = RawEventStore(dict(zip("xytp", cols))).load_event(0, len(cols[0]))
    m = gpu_map("A")[cols[1], cols[0]].astype(got.dtype)
    keep = (m[:, 0] >= 0) & (m[:, 0] < 37) & (m[:, 1] >= 0) & (m[:, 1] < 70)
    assert np.array_equal(got[:, 2:], plain[keep][:, 2:].astype(got.dtype))
    assert set(np.unique(got[:, 3])) == {0.0, 1.0}


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_rectified_events_lie_where_the_ideal_points_were(name):
    c = calib_of(name)
    H, W = c.sensor_size
    m = gpu_map(name)
    # L: the largest distance between the map's values at 8-neighbouring pixels
    L = 0.0
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = m[:H - dr, max(0, -dc):W - max(0, dc)]
        b = m[dr:, max(0, dc):W + min(0, dc)]
        L = max(L, float(np.sqrt(((a - b) ** 2).sum(-1)).max()))
    rs = np.random.RandomState(11)
    ideal = np.stack([rs.uniform(0, H, 4000), rs.uniform(0, W, 4000)], 1)
    sensor = np.rint(c.distort_points(ideal))                      # round to sensor pixels
    on = (sensor[:, 0] >= 0) & (sensor[:, 0] < H) & (sensor[:, 1] >= 0) & (sensor[:, 1] < W)
    ideal, sensor = ideal[on], sensor[on]
    n = len(ideal)
    cols = (sensor[:, 1].astype(np.int16), sensor[:, 0].astype(np.int16), np.arange(n, dtype=np.int32), np.ones(n, dtype=bool))
    got, n_sensor, n_image = run_events(cols, c)
    kept = got[:, 2] * 1e6                                           # t = the event's index: which ideal point a row belongs to
    idx = np.rint(kept).astype(np.int64)
    dist = np.sqrt(((got[:, :2] - ideal[idx]) ** 2).sum(-1))
    bound = 0.5 * np.sqrt(2.0) * L + 1e-9
    print(f"case {name}: {n} points, {len(got)} kept, L = {L:.4f} px, largest distance {dist.max():.4f} px, bound {bound:.4f} px")
    assert n_sensor == 0 and len(got) > n // 2 and dist.max() <= bound


# ------------------------------------------------------------------ undistort_events
@pytest.mark.parametrize("name", ["lens", "small"])
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_undistort_events_equals_the_reference_in_every_container(name, tag):
    ev, map_x, map_y, h, w, kept = R.golden_sets()[name]
    ev = ev.astype(np.float64 if tag == "f64" else np.float32)
    want = R.golden_output(ev, *kept[tag])
    assert np.array_equal(R.undistort_events(ev, map_x, map_y, h, w), want)
    got = utils.undistort_events(ev, map_x, map_y, h, w)                                             # numpy in -> numpy out
    assert isinstance(got, np.ndarray) and got.dtype == ev.dtype and np.array_equal(got, want)
    got = utils.undistort_events(torch.from_numpy(ev), torch.from_numpy(map_x), torch.from_numpy(map_y), h, w)   # CPU tensor
    assert isinstance(got, torch.Tensor) and not got.is_cuda and got.dtype == torch.from_numpy(ev).dtype and np.array_equal(got.numpy(), want)
    got = utils.undistort_events(torch.from_numpy(ev).to(DEV), map_x, map_y, h, w)                     # device tensor
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)


def test_undistort_events_edges():
    m = R.pixel_grid(5, 6)
    assert utils.undistort_events(np.zeros((0, 4)), m[..., 1], m[..., 0], 5, 6).shape == (0, 4)
    ev = np.array([[-1.0, -2.0, 0.1, 1.0], [4.9, 5.9, 0.2, 0.0]])                    # numpy's indexing: negative counts from the end
    assert np.array_equal(utils.undistort_events(ev, m[..., 1], m[..., 0], 5, 6), R.undistort_events(ev, m[..., 1], m[..., 0], 5, 6))
    for bad in ([5.0, 0.0], [0.0, 6.0], [-6.0, 0.0], [np.nan, 0.0], [0.0, 1e12]):
        with pytest.raises(IndexError):
            utils.undistort_events(np.array([bad + [0.0, 1.0]]), m[..., 1], m[..., 0], 5, 6)
    nan_map = m[..., 0].copy()
    nan_map[2, 3] = np.nan                                                           # a map value that is no int32: dropped
    got = utils.undistort_events(np.array([[2.0, 3.0, 0.0, 1.0], [1.0, 1.0, 0.0, 1.0]]), m[..., 1], nan_map, 5, 6)
    assert np.array_equal(got, [[1.0, 1.0, 0.0, 1.0]])


def test_the_store_undistorts_with_its_own_map():
    cols = raw_columns(500, "A", seed=4)
    store = RawEventStore(dict(zip("xytp", cols)), calibration=calib_of("A"))
    batch = store.load_event(0, 500)
    m = gpu_map("A")
    want = R.undistort_events(batch, m[..., 1], m[..., 0], 37, 70)
    got = store.undistort(batch)
    assert isinstance(got, np.ndarray) and 0 < len(want) < 500 and np.array_equal(got, want)


# ------------------------------------------------------------------ images
def frames(n, H, W, dtype, seed=0):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (n, H, W)).astype(np.uint8) if dtype == np.uint8 else rs.uniform(-3, 3, (n, H, W)).astype(np.float32)


HOMOGRAPHY = np.array([[0.95, 0.04, 1.5], [-0.03, 1.02, -0.8], [1e-4, -5e-5, 1.0]])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("case", ["A", "B-roi-aligned", "B-roi-unaligned", "C-border", "A-homography"])
def test_images_equal_the_restatement(case, dtype):
    name = case[0]
    H, W = R.CASES[name]["size"]
    K, D = R.case_K(name), R.CASES[name]["D"]
    roi = {"B-roi-aligned": (4, 60, 8, 88), "B-roi-unaligned": (3, 50, 5, 78)}.get(case)
    border = 7.4 if case == "C-border" else 0
    hom, dsize = (HOMOGRAPHY, (50, 30)) if case == "A-homography" else (None, None)
    src = frames(1, H, W, dtype, seed=len(case))[0]
    want = R.undistort_image(src, K, D, None, hom, dsize, roi, border)
    got = frame_warp.undistort_image(src, calib_of(name), hom, dsize, roi, border)
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
    print(f"{case} {np.dtype(dtype).name}: {int((got != want).sum())} of {want.size} pixels differ; {int((want == WR.border_as(dtype, border)).sum())} on the border value")
    assert np.array_equal(got, want)
    dev = frame_warp.undistort_image(torch.from_numpy(src).to(DEV), calib_of(name), hom, dsize, roi, border)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    if roi is not None:                                             # a pixel's bits do not depend on the rectangle
        full = frame_warp.undistort_image(src, calib_of(name))
        assert np.array_equal(full[roi[0]:roi[1], roi[2]:roi[3]], got)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_a_frame_alone_equals_the_frame_in_a_batch_of_3(dtype):
    c = calib_of("A")
    srcs = frames(3, 37, 70, dtype, seed=9)
    batch = utils.undistort_image_batch(srcs, c)
    assert batch.is_cuda and batch.shape == (3, 37, 70)
    for b in range(3):
        assert np.array_equal(batch[b].cpu().numpy(), R.undistort_image(srcs[b], c.K, c.D))
        assert np.array_equal(batch[b].cpu().numpy(), utils.undistort_image(srcs[b], c))
    out = torch.zeros((3, 40, 80), dtype=batch.dtype, device=DEV)   # into a view of a larger tensor (unaligned rows)
    utils.undistort_image_batch(srcs, c, out=out[:, 2:39, 3:73])
    assert torch.equal(out[:, 2:39, 3:73], batch) and not out[:, :2].any() and not out[:, :, :3].any()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_no_lens_returns_the_image_and_with_a_homography_the_perspective_warp(dtype):
    c = CameraCalibration(R.case_K("A"), np.zeros(5), (37, 70))
    src = frames(1, 37, 70, dtype, seed=2)[0]
    assert np.array_equal(frame_warp.undistort_image(src, c), src)
    for dsize, roi in (((50, 30), None), ((64, 40), (1, 38, 3, 60))):
        got = frame_warp.undistort_image(src, c, HOMOGRAPHY, dsize, roi, 3)
        assert np.array_equal(got, frame_warp.warp_perspective(src, HOMOGRAPHY, dsize, frame_warp.INTER_LINEAR, 3, roi))


def test_with_a_lens_and_a_homography_the_coordinates_are_the_two_steps():
    """One resample is not two: the fused kernel's PIXELS differ from ``warp_perspective(undistort(image))``, its COORDINATES are
    those of the two steps.  A ramp image returns the coordinate it is sampled at, on the 1/32 grid of the sampling: the fused result
    on a column ramp and a row ramp is compared with distort(M^-1 (c, r, 1)) computed in plain float64."""
    c = calib_of("B")
    H, W = c.sensor_size
    dsize = (80, 50)
    g = R.pixel_grid(H, W).astype(np.float32)
    v_img = frame_warp.undistort_image(g[..., 0].copy(), c, HOMOGRAPHY, dsize, border_value=-1000)
    u_img = frame_warp.undistort_image(g[..., 1].copy(), c, HOMOGRAPHY, dsize, border_value=-1000)
    rr, cc = np.meshgrid(np.arange(dsize[1], dtype=np.float64), np.arange(dsize[0], dtype=np.float64), indexing="ij")
    Minv = np.linalg.inv(HOMOGRAPHY)
    p = np.einsum("ij,jhw->ihw", Minv, np.stack([cc, rr, np.ones_like(cc)]))
    ideal = np.stack([p[1] / p[2], p[0] / p[2]], -1)                 # step 1: the perspective warp's source position (row, col)
    sensor = c.distort_points(ideal)                                 # step 2: where the lens put it
    inside = (sensor[..., 0] >= 0) & (sensor[..., 0] <= H - 1 - 1 / 32) & (sensor[..., 1] >= 0) & (sensor[..., 1] <= W - 1 - 1 / 32)
    err = max(float(np.abs(v_img - sensor[..., 0])[inside].max()), float(np.abs(u_img - sensor[..., 1])[inside].max()))
    bound = 1 / 64 + 1e-4                                            # half a step of the 1/32 grid + float32 blending of values < 100
    print(f"{int(inside.sum())} of {inside.size} pixels inside; largest coordinate difference {err:.5f} px, bound {bound:.5f} px")
    assert inside.sum() > inside.size // 2 and err <= bound
    assert np.array_equal(u_img, R.undistort_image(g[..., 1].copy(), c.K, c.D, None, HOMOGRAPHY, dsize, None, -1000))


# ------------------------------------------------------------------ composition
def plan_state(plan):
    """Every device tensor the plan holds, by field name, and the fraction layout the resident loops read."""
    import dataclasses

    found = {f.name: getattr(plan, f.name) for f in dataclasses.fields(plan) if isinstance(getattr(plan, f.name), torch.Tensor)}
    for k, t in enumerate(plan.frac_compact or ()):
        found[f"frac_compact[{k}]"] = t
    return found


def bits(t):
    return t.contiguous().view(torch.uint8)     # (padding slots hold NaN)


def test_a_rectified_plan_is_the_full_build_on_the_rectified_events():
    """``store.plan(.., rectify=True)`` holds the tensors of ``EventPlan.build`` on ``rectify_events_raw``'s output, bit for bit.
    The full build leaves the order of the events INSIDE a source pixel's run to its counting sort's atomic counter, so two builds of
    one array -- ``EventPlan.build`` called twice -- already differ there; the package's own normal form for comparing builds is
    ``canonical_runs`` (every run ordered by (dt, x, y)).  The event streams are compared in that form, with timestamps that are all
    different so that the order is total; offsets, the part table and the fraction layout (canonical by construction) as built."""
    from event_based_bos_amd.event_plan import canonical_runs

    cols = list(raw_columns(6000, "A", seed=6))
    cols[2] = (np.arange(6000) * 7 + 3).astype(np.int32)               # no two events share a timestamp
    c = calib_of("A")
    store = RawEventStore(dict(zip("xytp", cols)), calibration=c)
    plan = store.plan(100, 5100, (37, 70), rectify=True)
    ev, _, _ = calibration.rectify_events_raw(*(torch.from_numpy(col[100:5100]).to(DEV) for col in cols), c)
    want = EventPlan.build(ev, (37, 70), "first", True, "auto")
    assert plan.n == want.n == len(ev) and plan.tile == want.tile and plan.fractional
    a, b = plan_state(canonical_runs(plan)), plan_state(canonical_runs(want))
    a.update({k: v for k, v in plan_state(plan).items() if k.startswith("frac_compact")})
    b.update({k: v for k, v in plan_state(want).items() if k.startswith("frac_compact")})
    print(f"plan tensors compared: {sorted(a)}")
    assert set(a) == set(b) and {"x", "y", "dt", "p", "perm", "key_offsets", "frac_compact[4]"} <= set(a)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(store.load_event(100, 5100, rectify=True), ev.cpu().numpy())
    assert (ev[:, :2] != ev[:, :2].trunc()).any()                    # the events are off the grid


def test_contrast_maximization_runs_the_fractional_route_on_a_rectified_window():
    import event_based_bos_amd as ebos

    cols = raw_columns(20000, "A", seed=7)
    store = RawEventStore(dict(zip("xytp", cols)), calibration=calib_of("A"))
    events = store.load_event(0, 20000, rectify=True)
    cfg = {"method": "contrast_maximization", "warp_direction": "first", "motion_model": "dense-flow", "outer_padding": 0,
           "cost": "hybrid", "cost_with_weight": {"image_variance": 1.0, "flow_norm": 0.001},
           "iwe": {"method": "bilinear_vote", "blur_sigma": 1}, "patch": {"size": [10, 14], "sliding_window": [10, 14]},
           "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.1}}}
    solver = ebos.solver.ContrastMaximization((37, 70), (37, 70), solver_config=cfg)
    flow = solver.estimate(events)
    flow = flow.cpu().numpy() if isinstance(flow, torch.Tensor) else np.asarray(flow)
    assert flow.shape == (2, 37, 70) and np.isfinite(flow).all() and len(solver.history) >= 1 and np.isfinite(solver.history).all()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_frame_store_with_and_without_a_calibration(dtype):
    raw = frames(4, 37, 70, dtype, seed=8)
    ts = np.arange(4) * 1000 + 10
    no_lens = CameraCalibration(R.case_K("A"), np.zeros(5), (37, 70))
    lens = calib_of("A")
    roi = (2, 28, 4, 44)
    for hom, size in ((None, None), (HOMOGRAPHY, (30, 50))):
        plain = FrameStore(raw, ts, hom, size)
        same = FrameStore(raw, ts, hom, size, calibration=no_lens)
        rect = FrameStore(raw, ts, hom, size, calibration=lens)
        dsize = None if hom is None else (50, 30)
        today = raw[1] if hom is None else frame_warp.warp_perspective(raw[1], hom, dsize)
        assert np.array_equal(plain.load_image(1)[0], today)                                    # without one: today's output
        assert np.array_equal(same.load_image(1)[0], today)                                     # D = 0: likewise
        assert np.array_equal(rect.load_image(1)[0], R.undistort_image(raw[1], lens.K, lens.D, None, hom, dsize))
        r = roi if hom is None else (2, 28, 4, 44)
        b_plain, t_plain = plain.load_images([0, 1, 3], roi=r)
        b_same, _ = same.load_images([0, 1, 3], roi=r)
        b_rect, t_rect = rect.load_images([0, 1, 3], roi=r)
        assert torch.equal(b_plain, b_same) and np.array_equal(t_plain, t_rect)
        for k, i in enumerate((0, 1, 3)):
            assert np.array_equal(b_rect[k].cpu().numpy(), R.undistort_image(raw[i], lens.K, lens.D, None, hom, dsize, r))
