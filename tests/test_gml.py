"""CPU tests of the generative patch-pyramid solver: tests/_gml_ref.py (the torch float64 restatement that checks the HIP solver)
against the reference's fixture golden_gml.npz, and the solver's configuration surface and registries.  No GPU needed.

The reference's trajectory is sensitive to rounding (see tests/test_gpu_gml.py): the restatement follows it to 1e-12 at the first
iteration of every case and all the way through the 260 x 346 cases and the 720 x 1280 case, while on the 128 x 160 cases it parts
from it a few iterations into the second scale (differences in the gradient's summation order only).  Where it parts, the bounds
below are the measured spread of the two paths (per-iteration loss and output flow relative to max|flow|).
"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_cases as C  # noqa: E402
import _gml_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "golden_gml.npz"))
STABLE = ("yaml_260", "terms_260", "yaml_720")     # the restatement follows the reference through every iteration
PARTED_HIST, PARTED_FLOW = 0.1, 0.5                # measured: <= 5.1e-2 and <= 3.4e-1 on the 128 x 160 cases


@pytest.mark.parametrize("name", list(C.CASES))
def test_restatement_vs_reference(name):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    out = R.solve(frame, events, c["gml"], c["cost"], c["n_iter"], C.roi_of(name), c["init_seed"])
    loss, ref = out["history"]["loss"], GOLDEN[name + "_loss"]
    assert loss.shape == ref.shape
    assert abs(loss[0] - ref[0]) <= 1e-12 * abs(ref[0])
    for k in c["cost"]:
        r = GOLDEN[f"{name}_{k}"]
        assert abs(out["history"][k][0] - r[0]) <= 1e-12 * max(abs(r[0]), 1e-300), k
    # scale 1 runs through identical torch ops: its parameters agree
    assert np.abs(out["params"][0] - GOLDEN[name + "_x1"]).max() <= 1e-9
    rows = C.stored_rows(name)
    f = out["flow"] if rows is None else out["flow"][:, rows]
    fe = np.abs(f - GOLDEN[name + "_flow"]).max() / float(GOLDEN[name + "_flow_absmax"])
    d = np.abs(loss - ref) / np.abs(ref)
    if name in STABLE:
        assert d.max() <= 1e-9 and fe <= 1e-9, (d.max(), fe)
    else:
        assert d.max() <= PARTED_HIST and fe <= PARTED_FLOW, (d.max(), fe)


def test_fixture_margins_clear_of_rounding():
    for name in C.CASES:
        m = GOLDEN[name + "_margin"]
        assert len(m) == len(GOLDEN[name + "_loss"]) and m.min() > 1e-9


def test_iterations_per_scale():
    assert [600 // (R.FINEST_SCALE - s + 1) for s in range(1, 5)] == [120, 150, 200, 300]
    assert R.grid_shape(720, 1280, 64) == (12, 20) and R.grid_shape(260, 346, 8) == (33, 44)


def test_initial_potentials_reshape_layout():
    np.random.seed(3)
    x = R.initial_potentials(3, 2, 3)
    np.random.seed(3)
    np.random.random()
    draws = np.array([np.random.random() * 2 - 1 for _ in range(6)])
    flat = np.zeros(18)
    flat[::3] = draws
    assert np.array_equal(x, flat.reshape(3, 2, 3))
    assert x[1].any() and x[2].any()          # p_x, p_y do not start at zero


# ------------------------------------------------------------------ configuration surface (no GPU needed to construct)
def _make(**gml):
    import event_based_bos_amd as ebos
    return ebos.solver.collections["generative_patch_pyramid"]((128, 160), (128, 160), {}, C.solver_config("yaml_128", **gml))


def test_config_accepted():
    s = _make()
    assert s._gml_roi == (0, 128, 0, 160) and s._gml_n_dim == 3
    assert s.cost_func.get_history() == {"loss": [], "diff_norm": [], "image_gradient": [], "flow_norm_pxy": []}


@pytest.mark.parametrize("gml", [{"poisson_model": False}, {"angle_model": True}, {"sobel_ksize": 5}, {"model_image": "e2vid"}])
def test_not_implemented_options(gml):
    with pytest.raises(NotImplementedError):
        _make(**gml)


def test_not_implemented_optimizer_and_costs():
    import event_based_bos_amd as ebos
    cls = ebos.solver.collections["generative_patch_pyramid"]
    cfg = C.solver_config("yaml_128")
    cfg["optimizer"]["method"] = "SGD"
    with pytest.raises(NotImplementedError):
        cls((128, 160), (128, 160), {}, cfg)
    cfg = C.solver_config("yaml_128")
    cfg["cost_with_weight"]["total_variation"] = 1.0
    with pytest.raises(NotImplementedError):
        cls((128, 160), (128, 160), {}, cfg)
    cfg = C.solver_config("yaml_128", optimize_warp=False)
    with pytest.raises(ValueError):
        cls((128, 160), (128, 160), {}, cfg)   # flow_norm_pxy without optimize_warp


def test_registries():
    import event_based_bos_amd as ebos
    from event_based_bos_amd import solver
    assert solver.collections["generative_patch_pyramid"] is solver.GenerativePatchPyramid
    assert "patch_eklt_pyramid2" not in solver.collections
    assert solver.collections["contrast_maximization"] is solver.ContrastMaximization
    reg = types.SimpleNamespace(SolverBase=solver.SolverBase, collections={})
    cls = solver.register_generative_into(reg)
    assert set(reg.collections) == {"patch_eklt_pyramid2"} and reg.collections["patch_eklt_pyramid2"] is cls
    reg2 = types.SimpleNamespace(SolverBase=solver.SolverBase, collections={})
    solver.register_into(reg2)
    assert set(reg2.collections) == {"contrast_maximization", "cmax"}
    s = cls((64, 80), (64, 80), {}, {"optimizer": {"method": "Adam", "n_iter": 5}, "cost_with_weight": {"diff_norm": 1.0},
                                     "generative_ml": {"poisson_model": True, "optimize_warp": True, "model_image": "current"}})
    assert isinstance(s, solver.SolverBase) and s._gml_roi == (0, 64, 0, 80)
    assert ebos._hip.SIGNATURES["ebos_gml_solve_scale_f64"][0] is not None
