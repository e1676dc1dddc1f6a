"""The generative patch-pyramid solver on the GPU (csrc/gml.hip, event_based_bos_amd.solver.generative) against the torch float64
restatement tests/_gml_ref.py (itself pinned to the reference by tests/test_gml.py) and the reference's fixture golden_gml.npz.

Where the trajectories can be compared and where they cannot: the objective at a given x is a smooth function of the inputs except
for abs() at zero, and torch.gradient of the upsampled flow is zero up to rounding on the replicate-padded border bands, so the
sign that picks the image_gradient subgradient there is rounding noise in the reference itself.  Over hundreds of Adam steps such
differences grow (two torch-CPU evaluations that differ only in summation order part at about 1e-8 within a few steps of a new
scale).  So the first iteration of every window is compared at 1e-10; the whole history and the output flow at 1e-9 on the cases
whose path is stable (260 x 346, 720 x 1280), and with the bounds that tests/test_gml.py measures between the reference and its
restatement on the others.  Objective values and gradients at a given x agree to ~1e-15 (measured).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_cases as C  # noqa: E402
import _gml_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "golden_gml.npz"))
STABLE = ("yaml_260", "terms_260", "yaml_720")   # the reference's path is stable under rounding: compared at 1e-9 throughout
# where the paths part (the 128 x 160 cases, a few iterations into scale 2), the bounds of tests/test_gml.py: measured on an MI355X
# <= 3.8e-2 per-iteration loss and <= 2.6e-1 of max|flow|, the same spread as the CPU restatement's (<= 5.1e-2, <= 3.4e-1)
HIST_REL, FLOW_REL = 0.1, 0.5


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as ebos
    return ebos


def _solver(ebos, name, **gml):
    c = C.CASES[name]
    return ebos.solver.collections["generative_patch_pyramid"](c["shape"], c["shape"], {}, C.solver_config(name, **gml))


def _run(ebos, name, **gml):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    s = _solver(ebos, name, **gml)
    np.random.seed(c["init_seed"])
    flow = s.estimate(events, frame=frame, background=frame)
    return s, flow


def _objective_gpu(ebos, st, gml, cost, p, q, x):
    lib = ebos._hip.require_gpu()
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    H, W = st["gx"].shape
    gx, gy, qq, we, wi, xx = t(st["gx"]), t(st["gy"]), t(q), t(st["we"]), t(st["winv"]), t(x)
    mask = st["mask"]
    rows, cols = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    roi = (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1) if len(rows) else (0, 0, 0, 0)
    terms = ("diff_norm", "image_gradient", "flow_norm_pxy")
    w = torch.tensor([float(cost.get(k, 0.0)) for k in terms], dtype=torch.float64, device=dev)
    order = [terms.index(k) for k in cost]
    o = torch.tensor(order + [0] * (3 - len(order)), dtype=torch.int32, device=dev)
    parts = torch.zeros(4, dtype=torch.float64, device=dev)
    grad = torch.zeros_like(xx)
    nbytes = int(lib.ebos_gml_scratch_bytes(H, W, 8))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flags = (1 if gml.get("no_polarity") else 0) | (2 if we is not None else 0)
    p_ = ebos._hip.ptr
    ebos._hip.check(lib.ebos_gml_objective_f64(H, W, p, xx.shape[0], *roi, flags, p_(w), p_(o), len(order), p_(gx), p_(gy), p_(qq),
                                               p_(we), p_(wi), p_(xx), p_(parts), p_(grad), p_(scratch), nbytes,
                                               ebos._hip.stream_ptr()), "ebos_gml_objective_f64")
    torch.cuda.synchronize()
    return parts.cpu().numpy(), grad.cpu().numpy()


OBJ_CASES = ["yaml_128", "yaml_128_roi", "nowarp_128", "nopol_128", "evhist_128", "sigma0_log_128", "terms_260"]


@pytest.mark.parametrize("name", OBJ_CASES)
@pytest.mark.parametrize("p", [64, 16, 8])
def test_objective_and_gradient_vs_autograd(ebos, name, p):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    H, W = c["shape"]
    st = R.prepare(frame, R.polarity_image(events, (H, W)), c["gml"], C.roi_of(name))
    q = R.measured(st)
    gh, gw = R.grid_shape(H, W, p)
    nd = 3 if c["gml"]["optimize_warp"] else 1
    x = np.random.RandomState(7 + p).uniform(-1, 1, (nd, gh, gw))
    if nd == 3:
        x[1:] *= 0.8
    loss, terms, grad = R.objective_and_grad(st, c["gml"], c["cost"], p, q, x)
    parts, g = _objective_gpu(ebos, st, c["gml"], c["cost"], p, q, x)
    assert abs(parts[0] - loss) <= 1e-10 * abs(loss), (parts[0], loss)
    for k, v in terms.items():
        i = 1 + ("diff_norm", "image_gradient", "flow_norm_pxy").index(k)
        assert abs(parts[i] - v) <= 1e-10 * max(abs(v), 1e-300), (k, parts[i], v)
    e = np.linalg.norm(g - grad) / np.linalg.norm(grad)
    print(f"{name} p={p}: loss rel {abs(parts[0] - loss) / abs(loss):.1e}  grad rel-L2 {e:.1e}")
    assert e <= 1e-9, e


@pytest.mark.parametrize("name", [n for n in C.CASES if n != "yaml_720"])
def test_fixture_end_to_end(ebos, name):
    s, flow = _run(ebos, name)
    h = s.cost_func.get_history()
    ref = GOLDEN[name + "_loss"]
    loss = np.array(h["loss"])
    assert loss.shape == ref.shape
    assert abs(loss[0] - ref[0]) <= 1e-10 * abs(ref[0])
    for k in C.CASES[name]["cost"]:
        r = GOLDEN[f"{name}_{k}"]
        assert abs(h[k][0] - r[0]) <= 1e-10 * max(abs(r[0]), 1e-300), k
    d = np.abs(loss - ref) / np.abs(ref)
    rows = C.stored_rows(name)
    f = flow if rows is None else flow[:, rows]
    fe = np.abs(f - GOLDEN[name + "_flow"]).max() / float(GOLDEN[name + "_flow_absmax"])
    print(f"{name}: first {d[0]:.1e}  max {d.max():.1e}  last {d[-1]:.1e}  flow {fe:.1e}")
    if name in STABLE:
        assert d.max() <= 1e-9 and fe <= 1e-9
    else:
        assert d.max() <= HIST_REL and fe <= FLOW_REL
    assert flow.shape == (2,) + tuple(C.CASES[name]["shape"])
    xmin, xmax, ymin, ymax = C.roi_of(name)
    outside = flow.copy()
    outside[:, xmin:xmax, ymin:ymax] = 0
    assert not outside.any()


def test_720_case(ebos):
    name = "yaml_720"
    s, flow = _run(ebos, name)
    h = s.cost_func.get_history()
    ref = GOLDEN[name + "_loss"]
    d = np.abs(np.array(h["loss"]) - ref) / np.abs(ref)
    f = flow[:, C.stored_rows(name)]
    fe = np.abs(f - GOLDEN[name + "_flow"]).max() / float(GOLDEN[name + "_flow_absmax"])
    print(f"yaml_720: first {d[0]:.1e}  max {d.max():.1e}  flow {fe:.1e}")
    assert d[0] <= 1e-10 and d.max() <= 1e-9 and fe <= 1e-9


def test_two_runs_bit_identical(ebos):
    _, f1 = _run(ebos, "yaml_128_roi")
    s2, f2 = _run(ebos, "yaml_128_roi")
    _, f3 = _run(ebos, "yaml_128_roi")
    assert np.array_equal(f1, f2) and np.array_equal(f2, f3)


@pytest.mark.parametrize("gml", [{"model_image": "black"}, {"model_image": "background"}, {"iwe_sigma": 0},
                                 {"weight_loss_by_inverse_event_hist": False}, {"use_log_intensity": True},
                                 {"no_polarity": True, "weight_loss_by_event_hist": True}])
def test_options_first_iterations_vs_ref(ebos, gml):
    """Every in-scope option: the first Adam iterations of a window against the restatement (before the paths can part)."""
    name = "yaml_128_roi"
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    g = dict(c["gml"], **gml)
    cfg = C.solver_config(name, **gml)
    cfg["optimizer"]["n_iter"] = 10   # 2, 2, 3, 5 iterations
    s = ebos.solver.collections["generative_patch_pyramid"](c["shape"], c["shape"], {}, cfg)
    model_frame = np.zeros_like(frame) if g["model_image"] == "black" else frame
    np.random.seed(c["init_seed"])
    s.estimate(events, frame=frame, background=frame)
    ref = R.solve(model_frame, events, g, c["cost"], 10, C.roi_of(name), c["init_seed"])
    a, b = np.array(s.cost_func.get_history()["loss"]), ref["history"]["loss"]
    d = np.abs(a - b) / np.abs(b)
    print(gml, d)
    assert d[0] <= 1e-10 and d.max() <= 1e-6


def test_solver_surface(ebos):
    from event_based_bos_amd import solver
    assert solver.collections["generative_patch_pyramid"] is solver.GenerativePatchPyramid
    s, _ = _run(ebos, "nowarp_128")
    assert set(s.params_per_scale) == {1, 2, 3, 4}
    assert s.params_per_scale[4].shape == (1,) + R.grid_shape(128, 160, 8)
    pf = s.poisson_to_flow(s.params_per_scale[4][0])
    ref = R.sobel_patch(torch.from_numpy(s.params_per_scale[4][0])).numpy()
    assert np.allclose(pf, ref, rtol=0, atol=1e-14)
    # device events give the same result as numpy events
    c = C.CASES["nowarp_128"]
    frame, events = C.case_inputs("nowarp_128")
    s2 = _solver(ebos, "nowarp_128")
    np.random.seed(c["init_seed"])
    f2 = s2.estimate(torch.from_numpy(events).cuda(), frame=frame)
    np.random.seed(c["init_seed"])
    f1 = _solver(ebos, "nowarp_128").estimate(events, frame=frame)
    assert np.array_equal(f1, f2)


def test_run_gml_tool(tmp_path):
    """tools/run_gml.py on the synthetic BOS scene: the loss decreases and the flow points along the true displacement (measured on
    an MI355X: loss 1.87 -> 0.16 and a cosine of 0.99 with d inside the ROI at 128 x 160; the bound asserted is a positive cosine)."""
    import subprocess
    root = os.path.dirname(HERE)
    out = tmp_path / "run_gml.json"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "run_gml.py"), "--size", "128", "160", "--n_iter", "120",
                        "--json", str(out)], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    import json
    res = json.loads(out.read_text())
    print(res)
    assert res["loss_last"] < res["loss_first"]
    assert res["cosine_roi"] > 0.0
