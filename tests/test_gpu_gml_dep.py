"""The single-scale generative solver on the GPU (csrc/gml.hip ebos_gml_dep_*, event_based_bos_amd.solver.generative_dependent)
against the torch float64 restatement tests/_gml_dep_ref.py (itself pinned to the reference by tests/test_gml_dep.py) and the
reference's fixture golden_gml_dep.npz.

Objective values and gradients at a given x are compared to autograd at 1e-12.  Over many Adam steps the trajectories part where
the reference's own path is sensitive to rounding (abs() at zero in image_gradient on the replicate-padded border bands, see
tests/test_gpu_gml.py): the first iteration of every window is compared at 1e-10, the rest with the per-case bounds of
tests/test_gml_dep.py (the CPU restatement's measured drift from the reference, with headroom).
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_dep_cases as C  # noqa: E402
import _gml_dep_ref as D  # noqa: E402
import _gml_ref as R  # noqa: E402
from test_gml_dep import BOUNDS  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "golden_gml_dep.npz"))
TERMS = ("diff_norm", "image_gradient", "flow_norm_pxy")


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as ebos
    return ebos


def _run(ebos, name, cls=None):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    cls = cls or ebos.solver.collections["generative_patch_dependent"]
    s = cls(c["shape"], c["shape"], {}, C.solver_config(name))
    np.random.seed(c["init_seed"])
    flow = s.estimate(events, frame=frame, background=frame)
    return s, flow


def _objective_gpu(ebos, st, gml, cost, p, s, roi, idx, grid):
    lib = ebos._hip.require_gpu()
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    H, W = st["gx"].shape
    q = st["hist"] * st["we"] if st["we"] is not None else st["hist"]
    gx, gy, qq, we, wi, xx = t(st["gx"]), t(st["gy"]), t(q), t(st["we"]), t(st["winv"]), t(grid)
    gh, gw = D.grid_shape(H, W, p, s)
    sel = np.zeros(gh * gw, dtype=np.int32)
    sel[idx] = np.arange(1, len(idx) + 1)
    sel_t = torch.from_numpy(sel).to(dev)
    w = torch.tensor([float(cost.get(k, 0.0)) for k in TERMS], dtype=torch.float64, device=dev)
    order = [TERMS.index(k) for k in cost]
    o = torch.tensor(order + [0] * (3 - len(order)), dtype=torch.int32, device=dev)
    parts = torch.zeros(4, dtype=torch.float64, device=dev)
    grad = torch.zeros_like(xx)
    nbytes = int(lib.ebos_gml_dep_scratch_bytes(H, W, p, s, *roi, 0, 0))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flags = (1 if gml.get("no_polarity") else 0) | (2 if we is not None else 0) | (0 if gml.get("poisson_model") else 4)
    p_ = ebos._hip.ptr
    ebos._hip.check(lib.ebos_gml_dep_objective_f64(H, W, p, s, xx.shape[0], *roi, flags, p_(w), p_(o), len(order), p_(gx), p_(gy),
                                                   p_(qq), p_(we), p_(wi), p_(sel_t), p_(xx), p_(parts), p_(grad), p_(scratch), nbytes,
                                                   ebos._hip.stream_ptr()), "ebos_gml_dep_objective_f64")
    torch.cuda.synchronize()
    return parts.cpu().numpy(), grad.cpu().numpy()


OBJ_CASES = ["yaml_128", "yaml_128_roi", "nowarp_128", "vel_128", "vel_nowarp_128", "thres_128", "nopol_128", "evhist_128", "odd_128",
             "yaml_260"]


@pytest.mark.parametrize("name", OBJ_CASES)
def test_objective_and_gradient_vs_autograd(ebos, name):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    H, W = c["shape"]
    p, s, thr, thres = C.geometry(name)
    roi = C.roi_of(name)
    st = R.prepare(frame, R.polarity_image(events, (H, W)), c["gml"], roi)
    idx = D.select(events, H, W, p, s, roi, thr, thres)
    gh, gw = D.grid_shape(H, W, p, s)
    nd = D.n_dim(c["gml"])
    grid = np.random.RandomState(11).uniform(-1, 1, (nd, gh, gw))
    grid[nd - 2:] *= 0.8 if c["gml"]["optimize_warp"] else 1.0
    mask = np.zeros(gh * gw, dtype=bool)
    mask[idx] = True
    grid[:, ~mask.reshape(gh, gw)] = 0.0
    loss, terms, g_ref = D.objective_and_grad(st, c["gml"], c["cost"], p, s, roi, idx, grid)
    parts, g = _objective_gpu(ebos, st, c["gml"], c["cost"], p, s, roi, idx, grid)
    assert abs(parts[0] - loss) <= 1e-12 * abs(loss), (parts[0], loss)
    for k, v in terms.items():
        assert abs(parts[1 + TERMS.index(k)] - v) <= 1e-12 * max(abs(v), 1e-300), (k, parts[1 + TERMS.index(k)], v)
    e = np.linalg.norm(g - g_ref) / np.linalg.norm(g_ref)
    print(f"{name}: loss rel {abs(parts[0] - loss) / abs(loss):.1e}  grad rel-L2 {e:.1e}")
    assert e <= 1e-12, e
    assert not g[:, ~mask.reshape(gh, gw)].any()   # unselected cells: zero gradient


@pytest.mark.parametrize("name", list(C.CASES))
def test_fixture_end_to_end(ebos, name):
    c = C.CASES[name]
    s, flow = _run(ebos, name)
    gh, gw = s.patch_image_size
    sel = np.unpackbits(GOLDEN[name + "_selected"])[:gh * gw].astype(bool)
    assert np.array_equal(s.estimate_indices, np.nonzero(sel)[0])
    h = s.cost_func.get_history()
    ref = GOLDEN[name + "_loss"]
    loss = np.array(h["loss"])
    assert loss.shape == ref.shape
    assert abs(loss[0] - ref[0]) <= 1e-10 * abs(ref[0])
    for k in c["cost"]:
        assert abs(h[k][0] - GOLDEN[f"{name}_{k}"][0]) <= 1e-10 * max(abs(GOLDEN[f"{name}_{k}"][0]), 1e-300), k
    d = np.abs(loss - ref) / np.abs(ref)
    amax = float(GOLDEN[name + "_flow_absmax"])
    fe = np.abs(flow[:, C.stored_rows(name)] - GOLDEN[name + "_flow"]).max() / amax
    x = s.params
    xr = GOLDEN[name + "_x"]
    xe = np.abs(x[:, C.stored_param_rows(name)] - xr).max() / max(np.abs(xr).max(), 1e-300)
    print(f"{name}: loss first {d[0]:.1e} max {d.max():.1e}  flow {fe:.1e}  x {xe:.1e}")
    hb, fb = BOUNDS[name]
    assert d.max() <= hb and fe <= fb and xe <= fb, (d.max(), fe, xe)
    assert flow.shape == (2,) + tuple(c["shape"]) and x.shape[0] == D.n_dim(c["gml"])
    assert not x[:, ~sel.reshape(gh, gw)].any()


def test_two_runs_bit_identical(ebos):
    s1, f1 = _run(ebos, "thres_128")
    s2, f2 = _run(ebos, "thres_128")
    assert np.array_equal(f1, f2) and np.array_equal(s1.params, s2.params)
    assert s1.cost_func.get_history() == s2.cost_func.get_history()


def test_registered_class_through_a_registry(ebos):
    from event_based_bos_amd import solver
    reg = types.SimpleNamespace(SolverBase=solver.SolverBase, collections={})
    cls = solver.register_dependent_into(reg)
    assert set(reg.collections) == {"patch_eklt_dependent"}
    s, f = _run(ebos, "yaml_128_roi", reg.collections["patch_eklt_dependent"])
    assert isinstance(s, solver.SolverBase) and isinstance(s, cls)
    _, f0 = _run(ebos, "yaml_128_roi")
    assert np.array_equal(f, f0)
