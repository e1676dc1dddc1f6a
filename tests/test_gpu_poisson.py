"""GPU checks of the Poisson integration (event_based_bos_amd/poisson.py, csrc/poisson.hip): every case of
tests/golden/golden_poisson.npz through the numpy and tensor APIs, the reference geometries against the restatement, batching and
determinism, strided inputs, boundaries, the constant flow, validation and WindowPipeline(poisson=True)."""
import os

import numpy as np
import pytest
import torch

from _poisson_cases import CASES, case_inputs, golden_case, synth_flow
from _poisson_ref import restated_image, restated_poisson, standardized

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_poisson.npz")
DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _po():
    from event_based_bos_amd import poisson
    return poisson


def rel_err(got, want, absmax=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / (np.abs(want).max() if absmax is None else absmax)


def assert_matches(P, want, name="", absmax=None):
    """float64: 1e-11 of max|P|; float32: within one ulp of the fixture."""
    assert P.dtype == want.dtype, name
    if want.dtype == np.float64:
        assert rel_err(P, want, absmax) <= 1e-11, (name, rel_err(P, want, absmax))
    else:
        ulps = np.abs(P.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        same_sign = np.sign(P) == np.sign(want)
        assert (ulps[same_sign] <= 1).all() and np.array_equal(P[~same_sign], want[~same_sign]), name


def assert_image_matches(img, want_u8, want_P, name=""):
    """uint8 equal, except pixels whose reference value before truncation lies within 1e-9 of an integer: those may differ by one
    and are fewer than 1e-4 of the pixels.  ``want_P``: the whole field the unrounded values are formed from."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape == want_u8.shape, name
    diff = img.astype(np.int32) - want_u8.astype(np.int32)
    if not diff.any():
        return
    v = standardized(want_P).astype(np.float64)
    near = np.abs(v - np.rint(v)) <= 1e-9
    assert (np.abs(diff) <= 1).all() and near[diff != 0].all(), name
    assert (diff != 0).sum() < max(1, 1e-4 * img.size), (name, int((diff != 0).sum()))


def _fixture_field(golden, name, flow, boundary):
    """The whole field to judge uint8 ties with: the reference's own where the fixture keeps every row; else the restatement,
    which tests/test_poisson.py pins to the reference's stored rows (1e-12 of max|P|) and whole uint8 picture."""
    rows, P, _, _ = golden_case(golden, name)
    return P if isinstance(rows, slice) else restated_poisson(flow[1], flow[0], boundary)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_numpy(golden, name):
    po = _po()
    flow, boundary = case_inputs(name)
    rows, want, u8, absmax = golden_case(golden, name)
    P = po.poisson_reconstruct(flow[1], flow[0], boundary)   # the visualizer's component views, numpy in -> numpy out
    assert isinstance(P, np.ndarray) and P.shape == boundary.shape
    assert_matches(P[rows], want, name, absmax)
    assert abs(float(np.abs(P).max()) - absmax) <= (1e-11 if P.dtype == np.float64 else 1.2e-7) * absmax
    img = po.poisson_image(flow, boundary).cpu().numpy()[0]
    assert_image_matches(img, u8, _fixture_field(golden, name, flow, boundary), name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_tensor(golden, name):
    po = _po()
    flow, boundary = case_inputs(name)
    rows, want, _, absmax = golden_case(golden, name)
    f = torch.from_numpy(flow).to(DEV)
    b = torch.from_numpy(boundary).to(DEV)
    P = po.poisson_reconstruct(f[1], f[0], b)   # (views of one device tensor: read in place)
    assert isinstance(P, torch.Tensor) and P.is_cuda
    assert_matches(P.cpu().numpy()[rows], want, name, absmax)
    Pb = po.poisson_reconstruct_batch(f, b)
    assert torch.equal(Pb[0], P)


@pytest.mark.parametrize("hw", [(640, 720), (720, 1280)])
def test_reference_geometries_against_the_restatement(hw):
    po = _po()
    H, W = hw
    flow = synth_flow(H, W, seed=H + W)
    P = po.poisson_reconstruct(flow[1], flow[0], np.zeros((H, W)))
    want = restated_poisson(flow[1], flow[0], np.zeros((H, W)))
    assert rel_err(P, want) <= 1e-11, rel_err(P, want)
    img = po.poisson_image(flow).cpu().numpy()[0]
    assert_image_matches(img, restated_image(want), want)


def test_batch_equals_single_calls_and_runs_are_bit_identical():
    po = _po()
    H, W = 131, 203
    flows = np.stack([synth_flow(H, W, seed=100 + k) for k in range(8)])
    bnd = np.random.RandomState(7).uniform(-1, 1, (8, H, W))
    f = torch.from_numpy(flows).to(DEV)
    b = torch.from_numpy(bnd).to(DEV)
    batch = po.poisson_reconstruct_batch(f, b)
    again = po.poisson_reconstruct_batch(f, b)
    assert torch.equal(batch, again)
    for k in range(8):
        one = po.poisson_reconstruct_batch(f[k], b[k])
        assert torch.equal(one[0], batch[k]), k
    imgs = po.poisson_image(f, b)
    for k in range(8):
        assert torch.equal(po.poisson_image(f[k], b[k])[0], imgs[k]), k


def test_strided_inputs():
    po = _po()
    H, W = 97, 150
    big = torch.from_numpy(synth_flow(200, 300, seed=3)).to(DEV)
    roi = big[:, 50:50 + H, 100:100 + W]                      # an ROI slice of a larger tensor, read in place
    assert not roi.is_contiguous()
    want = po.poisson_reconstruct_batch(roi.contiguous())
    assert torch.equal(po.poisson_reconstruct_batch(roi), want)
    assert torch.equal(po.poisson_reconstruct(roi[1], roi[0], torch.zeros((H, W), dtype=torch.float64, device=DEV)), want[0])
    arr = synth_flow(H, W, seed=4)                            # the component views of a [2, H, W] numpy array
    P = po.poisson_reconstruct(arr[1], arr[0], np.zeros((H, W)))
    np.testing.assert_array_equal(P, po.poisson_reconstruct_batch(np.ascontiguousarray(arr)).cpu().numpy()[0])
    assert rel_err(P, restated_poisson(arr[1], arr[0], np.zeros((H, W)))) <= 1e-11
    t = torch.from_numpy(np.ascontiguousarray(arr.transpose(0, 2, 1))).to(DEV).transpose(1, 2)   # a non-unit column stride: copied
    assert t.stride(-1) != 1
    assert torch.equal(po.poisson_reconstruct_batch(t), po.poisson_reconstruct_batch(t.contiguous()))


def test_non_zero_boundary():
    po = _po()
    H, W = 70, 90
    flow = synth_flow(H, W, seed=8)
    rs = np.random.RandomState(9)
    bnd = rs.uniform(-3, 3, (H, W))
    P = po.poisson_reconstruct(flow[1], flow[0], bnd)
    want = restated_poisson(flow[1], flow[0], bnd)
    assert rel_err(P, want) <= 1e-11
    np.testing.assert_array_equal(P[0], bnd[0])
    np.testing.assert_array_equal(P[-1], bnd[-1])
    np.testing.assert_array_equal(P[:, 0], bnd[:, 0])
    np.testing.assert_array_equal(P[:, -1], bnd[:, -1])
    # one boundary broadcast over a batch equals the per-item boundary
    f2 = torch.from_numpy(np.stack([flow, synth_flow(H, W, seed=10)])).to(DEV)
    b = torch.from_numpy(bnd).to(DEV)
    assert torch.equal(po.poisson_reconstruct_batch(f2, b), po.poisson_reconstruct_batch(f2, b.expand(2, H, W).contiguous()))
    img = po.poisson_image(flow, bnd).cpu().numpy()[0]
    assert_image_matches(img, restated_image(want), want)


def test_constant_flow_gives_an_exact_zero_field():
    po = _po()
    H, W = 48, 77
    for dt in (np.float32, np.float64):
        flow = np.empty((2, H, W), dtype=dt)
        flow[0], flow[1] = 1.75, -0.5          # a 2-DoF translation as a dense flow
        P = po.poisson_reconstruct(flow[1], flow[0], np.zeros((H, W), dtype=dt))
        assert P.dtype == dt and not P.any()
        img = po.poisson_image(flow).cpu().numpy()
        assert (img == 128).all()


def test_validation_errors():
    po = _po()
    f = torch.zeros((2, 4, 5), device=DEV)
    with pytest.raises(ValueError):
        po.poisson_reconstruct_batch(torch.zeros((2, 2, 5), device=DEV))
    with pytest.raises(ValueError):
        po.poisson_reconstruct_batch(torch.zeros((1, 2, 4, 2), device=DEV))
    with pytest.raises(ValueError):
        po.poisson_reconstruct_batch(f.to(torch.int32))
    with pytest.raises(ValueError):
        po.poisson_reconstruct_batch(f.half())
    with pytest.raises(ValueError):
        po.poisson_reconstruct_batch(f, torch.zeros((3, 4, 5), device=DEV))
    with pytest.raises(ValueError):
        po.poisson_reconstruct(f[1], f[0], torch.zeros((4, 6), device=DEV))
    with pytest.raises(ValueError):
        po.poisson_image(f, dtype=torch.float16)
    from event_based_bos_amd import _hip
    lib = _hip.require_gpu()
    need = int(lib.ebos_poisson_scratch_bytes(1, 4, 5))
    assert need > 0 and lib.ebos_poisson_scratch_bytes(1, 2, 5) == 0
    out = torch.empty((1, 4, 5), dtype=torch.float32, device=DEV)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.ebos_poisson_reconstruct(0, 0, 1, 4, 5, f.data_ptr(), 40, 20, 5, None, 0, 0, out.data_ptr(), 20, 5, None,
                                      scratch.data_ptr(), need - 8, None)
    assert rc == -4   # EBOS_ERR_SCRATCH
    rc = lib.ebos_poisson_reconstruct(0, 0, 1, 2, 5, f.data_ptr(), 40, 20, 5, None, 0, 0, out.data_ptr(), 20, 5, None,
                                      scratch.data_ptr(), need, None)
    assert rc == -1   # EBOS_ERR_INVALID_ARG
    rc = lib.ebos_poisson_reconstruct(2, 0, 1, 4, 5, f.data_ptr(), 40, 20, 5, None, 0, 0, out.data_ptr(), 20, 5, None,
                                      scratch.data_ptr(), need, None)
    assert rc == -1


def _pipeline_setup():
    import yaml

    import event_based_bos_amd as ebos

    h, w = 260, 346
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cmax_hot_plate1.yaml")))["solver"]
    cfg.update(patch={"size": [20, 26], "sliding_window": [20, 26]}, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.01},
               iwe={"method": "bilinear_vote", "blur_sigma": 0}, optimizer={"method": "Adam", "n_iter": 30, "parameters": {"lr": 0.05}})
    solver = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    rs = np.random.RandomState(5)
    n, k_win = 20_000, 3
    store = ebos.data_loader.RawEventStore({"x": rs.randint(0, w, n * k_win).astype(np.int16),
                                            "y": rs.randint(0, h, n * k_win).astype(np.int16),
                                            "t": np.sort(rs.randint(0, 8000 * k_win, n * k_win)).astype(np.int32) + 1_000_000,
                                            "p": rs.randint(0, 2, n * k_win).astype(bool)})
    return ebos, solver, store, [(i * n, (i + 1) * n) for i in range(k_win)]


def test_window_pipeline_poisson_images():
    ebos, solver, store, windows = _pipeline_setup()
    pipe = ebos.solver.WindowPipeline(solver, n_concurrent=2, poisson=True)
    flows = pipe.run(store, windows)
    assert len(pipe.poisson_images) == len(flows) == len(windows)
    want = _po().poisson_reconstruct_batch(np.stack(flows)).cpu().numpy()
    for k, (f, P) in enumerate(zip(flows, pipe.poisson_images)):
        assert f.dtype == np.float64 and P.dtype == np.float64 and P.shape == f.shape[1:]
        np.testing.assert_array_equal(P, want[k])
        assert np.abs(P).max() > 0
    plain = ebos.solver.WindowPipeline(solver, n_concurrent=2)
    assert plain.poisson_images is None
    flows2 = plain.run(store, windows)
    assert plain.poisson_images is None and len(flows2) == len(windows)
