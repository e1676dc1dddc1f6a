"""CPU tests of the single-scale generative solver (patch_eklt_dependent): tests/_gml_dep_ref.py (the torch float64 restatement that
checks the HIP solver) against the reference's fixture golden_gml_dep.npz, and the solver's configuration surface and registries.
No GPU needed.

Unlike the pyramid's 128 x 160 cases, the reference's path here is stable under rounding on every case: the restatement follows it
to <= 3e-13 (measured: per-iteration loss <= 1.9e-15 relative, flow <= 1e-14 of max|flow|, final parameters <= 2.9e-13 of their
max).  BOUNDS (per-iteration loss; flow and parameters relative to their max) are what the restatement and the GPU solver are
held to.  The GPU follows the fixture to 1e-9 except on the direct-velocity cases, which start from x = 0: there the first
iteration agrees to 3e-16 and the path then parts at ~5e-9 from the third step on, as on the pyramid's unstable cases (rounding
noise in the upsampled flow's torch.gradient picks the image_gradient subgradient on the replicate-padded bands).  Measured on an
MI355X: vel_128 2.5e-8 per iteration, 1.8e-7 of max|flow|, 6.6e-7 of the parameters; vel_nowarp_128 1.9e-9, 3.5e-8, 5.1e-8.
Their bounds keep more than 10x headroom over that.
"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_dep_cases as C  # noqa: E402
import _gml_dep_ref as D  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "golden_gml_dep.npz"))
BOUNDS = {name: (1e-9, 1e-9) for name in C.CASES}
BOUNDS.update({"vel_128": (1e-6, 1e-5), "vel_nowarp_128": (1e-6, 1e-5)})


def _selected(name, gh, gw):
    return np.nonzero(np.unpackbits(GOLDEN[name + "_selected"])[:gh * gw])[0]


@pytest.mark.parametrize("name", list(C.CASES))
def test_restatement_vs_reference(name):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    p, s, thr, thres = C.geometry(name)
    out = D.solve(frame, events, c["gml"], c["cost"], c["n_iter"], C.roi_of(name), p, s, thr, thres, c["init_seed"])
    gh, gw = D.grid_shape(*c["shape"], p, s)
    assert np.array_equal(out["indices"], _selected(name, gh, gw))
    loss, ref = out["history"]["loss"], GOLDEN[name + "_loss"]
    assert loss.shape == ref.shape
    assert abs(loss[0] - ref[0]) <= 1e-12 * abs(ref[0])
    for k in c["cost"]:
        r = GOLDEN[f"{name}_{k}"]
        assert np.abs(out["history"][k] - r).max() <= 1e-9 * max(np.abs(r).max(), 1e-300), k
    hb, fb = BOUNDS[name]
    d = np.abs(loss - ref) / np.abs(ref)
    fe = np.abs(out["flow"][:, C.stored_rows(name)] - GOLDEN[name + "_flow"]).max() / float(GOLDEN[name + "_flow_absmax"])
    xr = GOLDEN[name + "_x"]
    xe = np.abs(out["params"][:, C.stored_param_rows(name)] - xr).max() / np.abs(xr).max()
    assert d.max() <= hb and fe <= fb and xe <= fb, (d.max(), fe, xe)


def test_fixture_margins_clear_of_rounding():
    for name in C.CASES:
        m = GOLDEN[name + "_margin"]
        assert len(m) == len(GOLDEN[name + "_loss"]) == C.CASES[name]["n_iter"] and m.min() > 1e-9


def test_thresholding_drops_patches():
    c = C.CASES["thres_128"]
    gh, gw = D.grid_shape(*c["shape"], 4, 2)
    n_roi = len(_selected("yaml_128_roi", gh, gw))   # same ROI, no thresholding
    assert len(_selected("thres_128", gh, gw)) < n_roi // 2


def test_grid_geometry():
    # prepare_patch: centres arange(0, L - p + s, s) + p / 2; pad int(p / 2 // s) + 1; centre crop of the upsampled canvas
    assert D.axis(128, 4, 2)[1:] == (63, 2, 3)
    assert D.axis(128, 5, 3)[1:] == (42, 1, 2)
    assert D.grid_shape(720, 1280, 4, 2) == (359, 639)
    from event_based_bos_amd.solver.generative_dependent import DepAxis
    for L, p, s in ((128, 4, 2), (128, 5, 3), (346, 4, 2), (160, 8, 8), (131, 7, 2)):
        a = DepAxis(L, p, s)
        _, g, k, off = D.axis(L, p, s)
        assert (a.g, a.k, a.off) == (g, k, off)
    a = DepAxis(128, 5, 3)
    assert (a.lo[0], a.hi[0]) == (0, 4) and (a.lo[1], a.hi[1]) == (2, 7)   # int() truncates toward zero; odd p: 4-row first box
    b = a.boxes(10, 117)
    assert b.shape == (42, 3) and b[:, 2].sum() == np.count_nonzero((a.centres >= 10) & (a.centres <= 117))


def test_initial_vector_layout():
    np.random.seed(3)
    x = D.initial_vector({"poisson_model": True, "optimize_warp": True}, 4)
    np.random.seed(3)
    np.random.random()
    draws = np.random.random(4) * 2. - 1
    assert np.array_equal(x.reshape(-1, 3).T[0], draws) and not x.reshape(-1, 3).T[1:].any()
    assert not D.initial_vector({"poisson_model": False, "optimize_warp": True}, 5).any()


# ------------------------------------------------------------------ configuration surface (no GPU needed to construct)
def _cfg(name="yaml_128", **gml):
    return C.solver_config(name, **gml)


def _make(cfg, shape=(128, 160)):
    import event_based_bos_amd as ebos
    return ebos.solver.collections["generative_patch_dependent"](shape, shape, {}, cfg)


def test_config_accepted():
    s = _make(_cfg())
    assert s._gml_roi == (0, 128, 0, 160) and s._gml_n_dim == 3 and s.patch_image_size == (63, 79)
    assert s.cost_func.get_history() == {"loss": [], "diff_norm": [], "image_gradient": [], "flow_norm_pxy": []}
    assert s.estimate_indices.size == 0 and s.params is None
    assert _make(_cfg(poisson_model=False))._gml_n_dim == 4
    v = _make(_cfg("vel_nowarp_128"))
    assert v._gml_n_dim == 2 and v._gml_velocity


@pytest.mark.parametrize("gml", [{"angle_model": True}, {"sobel_ksize": 5}, {"model_image": "e2vid"}])
def test_not_implemented_options(gml):
    with pytest.raises(NotImplementedError):
        _make(_cfg(**gml))


def test_not_implemented_optimizer_and_costs():
    cfg = _cfg()
    cfg["optimizer"]["method"] = "SGD"
    with pytest.raises(NotImplementedError):
        _make(cfg)
    cfg = _cfg()
    cfg["cost_with_weight"]["total_variation"] = 1.0
    with pytest.raises(NotImplementedError):
        _make(cfg)


def test_value_errors():
    with pytest.raises(ValueError):
        _make(_cfg(model_image="black"))
    with pytest.raises(ValueError):
        _make(_cfg(optimize_warp=False))   # flow_norm_pxy without optimize_warp
    cfg = _cfg()
    cfg["patch_eklt"]["patch_size"] = 200   # larger than the image: no grid, no centre crop
    with pytest.raises(ValueError):
        _make(cfg)
    cfg = _cfg()
    cfg["filter"]["parameters"].update({"xmin": 10, "xmax": 11})
    with pytest.raises(ValueError):
        _make(cfg)


def test_registries():
    import event_based_bos_amd as ebos
    from event_based_bos_amd import solver
    assert solver.collections["generative_patch_dependent"] is solver.GenerativePatchDependent
    assert solver.collections["generative_patch_pyramid"] is solver.GenerativePatchPyramid
    assert "patch_eklt_dependent" not in solver.collections
    reg = types.SimpleNamespace(SolverBase=solver.SolverBase, collections={})
    cls = solver.register_dependent_into(reg)
    assert set(reg.collections) == {"patch_eklt_dependent"} and reg.collections["patch_eklt_dependent"] is cls
    s = cls((64, 80), (64, 80), {}, {"optimizer": {"method": "Adam", "n_iter": 5}, "cost_with_weight": {"diff_norm": 1.0},
                                     "generative_ml": {"poisson_model": True, "optimize_warp": True, "model_image": "current"},
                                     "patch_eklt": {"patch_size": 4, "sliding_window": 2, "do_event_thresholding": False}})
    assert isinstance(s, solver.SolverBase) and s._gml_roi == (0, 64, 0, 80) and s.patch_image_size == (31, 39)
    for n in ("ebos_gml_dep_scratch_bytes", "ebos_gml_dep_select", "ebos_gml_dep_init_f64", "ebos_gml_dep_objective_f64",
              "ebos_gml_dep_solve_f64"):
        assert n in ebos._hip.SIGNATURES
