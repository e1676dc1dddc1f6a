"""CPU checks of the sampled EKLT solvers (event_based_bos_amd.solver.eklt_sweep): tests/_eklt_ref.py -- the plain numpy
restatement of the reference's objective, samplers and ``estimate`` that checks the HIP sweep on the GPU (tests/test_gpu_eklt.py) --
against tests/golden/golden_eklt.npz, which tests/golden/make_golden_eklt.py wrote by running the reference itself; the package's
sampler tables, its refusals, its registration, and the host-only entries of the C ABI.  The fixture is ``shimmed``: OpenCV and
optuna are absent where it is made (see the generator).
"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eklt_cases as C  # noqa: E402
import _eklt_ref as E  # noqa: E402
from _eklt_warp64 import shift_and_weights, translation, warp_perspective_f64  # noqa: E402

from event_based_bos_amd.solver import GenerativeGlobal, GenerativePatchIndependent, register_eklt_into  # noqa: E402
from event_based_bos_amd.solver import eklt_sweep as S  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "golden_eklt.npz"))
COST_RTOL = 1e-13
INPLACE = ("p5s3_inplace",)   # the cases whose fixture holds the reference's in-place division of overlapping patches


def boxes_of(name):
    c = C.CASES[name]
    H, W = c["shape"]
    if c["kind"] == "global":
        return np.array([C.roi_of(name)])
    return E.patch_boxes(H, W, c["patch"]["patch_size"], c["patch"]["sliding_window"])


_TABLES = {}


def restated_table(name, inplace=None):
    """(cost [P, K], evaluated [P], bar [P, K], hyp4) of the case's explicit table, computed once and shared."""
    inplace = (name in INPLACE) if inplace is None else inplace
    if (name, inplace) not in _TABLES:
        c = C.CASES[name]
        frame, events = C.case_inputs(name)
        st = E.state(frame, events, c["gml"], C.roi_of(name))
        hyp4 = E.unfold(c["gml"], list(c["params"]), C.hypotheses(name))
        cost, ok, bar = E.cost_table(st, c["gml"], boxes_of(name), hyp4, 1.0, None, inplace, want_bar=True)
        for a in (cost, ok, bar, hyp4):
            a.setflags(write=False)
        _TABLES[(name, inplace)] = (cost, ok, bar, hyp4)
    return _TABLES[(name, inplace)]


def zero_norm_index(name):
    z = C.ZERO_NORM_BOX.get(name)
    return None if z is None else int(np.nonzero((boxes_of(name) == np.array(z)).all(axis=1))[0][0])


def test_fixture_is_shimmed_and_complete():
    assert int(GOLDEN["shimmed"]) == 1
    for name in C.CASES:
        assert GOLDEN[name + "_cost"].shape == (len(boxes_of(name)), C.CASES[name]["k"])
        assert float(GOLDEN[name + "_margin"]) > 1e-9


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restated_objective_equals_the_reference(name):
    want = GOLDEN[name + "_cost"]
    cost, ok, _, _ = restated_table(name)
    assert np.array_equal(np.isnan(cost), np.isnan(want))
    assert np.array_equal(ok, ~np.isnan(want).all(axis=1))
    m = ~np.isnan(want)
    rel = np.abs(cost[m] - want[m]) / np.abs(want[m])
    print(f"{name}: worst relative difference {rel.max():.2e}")
    assert rel.max() <= COST_RTOL


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restated_estimate_equals_the_reference(name):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    np.random.seed(c["init_seed"])
    if c["kind"] == "patch":
        flow, ok, best, _, _ = E.estimate_patch(frame, events, C.solver_config(name), inplace=name in INPLACE)
    else:
        flow, ok, best, _, _ = E.estimate_global(frame, events, C.solver_config(name))
    sel = np.unpackbits(GOLDEN[name + "_selected"])[:len(ok)].astype(bool)
    want_best = GOLDEN[name + "_best"].astype(np.int64)
    z = zero_norm_index(name)
    if z is not None:   # the reference divides by zero there: it optimises the box, this package does not
        assert sel[z] and not ok[z] and want_best[z] == -1
        sel[z] = False
    assert np.array_equal(ok, sel)
    assert np.array_equal(best, want_best)
    assert np.array_equal(flow[:, C.stored_rows(name)], GOLDEN[name + "_flow"])
    assert np.abs(flow).max() == float(GOLDEN[name + "_flow_absmax"])


def test_thresholding_drops_most_patches_and_keeps_a_zero_histogram_box():
    sel = np.unpackbits(GOLDEN["thres_selected"])[:96].astype(bool)
    assert 0 < sel.sum() < 24 and sel[zero_norm_index("thres")]


# ------------------------------------------------------------------ the documented differences
def test_in_place_division_of_overlapping_patches_is_the_only_difference():
    """Overlap without event-hist weights: the reference divides a view of its cached histogram, patch after patch.  Normalising
    the untouched histogram agrees with it on the first patch and departs on later ones; with event-hist weights (or
    slide = patch) the two are the same computation."""
    want = GOLDEN["p5s3_inplace_cost"]
    untouched = restated_table("p5s3_inplace", inplace=False)[0]
    rel = np.abs(untouched - want) / np.abs(want)
    assert rel[0].max() <= COST_RTOL and rel.max() > 1e-6
    for name in ("p5s3_we", "p8_k67"):
        assert np.array_equal(restated_table(name, inplace=True)[0], restated_table(name, inplace=False)[0])


def test_zero_norm_box_is_not_evaluated():
    cost, ok, _, _ = restated_table("thres")
    z = zero_norm_index("thres")
    assert not ok[z] and np.isnan(cost[z]).all() and ok.sum() > 0


# ------------------------------------------------------------------ the warp is one shift and four weights
@pytest.mark.parametrize("p", [(0.0, 0.0), (1.0, -2.0), (-31.0 / 32.0, 1.0 / 32.0), (2.6, -2.6), (-2.6, 2.6), (0.37, -1.93)])
def test_translation_is_one_shift_and_four_weights(p):
    rs = np.random.RandomState(3)
    g = rs.normal(size=(21, 37))
    full = warp_perspective_f64(g, translation(*p), (37, 21))
    sr, sc, (w00, w01, w10, w11) = shift_and_weights(*p)
    pad = np.zeros((21 + 12, 37 + 12))
    pad[6:27, 6:43] = g
    at = lambda dr, dc: pad[6 + sr + dr:27 + sr + dr, 6 + sc + dc:43 + sc + dc]
    assert np.array_equal(full, ((at(0, 0) * w00 + at(0, 1) * w01) + at(1, 0) * w10) + at(1, 1) * w11)


# ------------------------------------------------------------------ sampler tables
def _opt(sampler, n, params):
    return {"method": "optuna", "sampler": sampler, "n_iter": n, "parameters": params}


def test_random_table_is_numpys_draws():
    opt = _opt("random", 9, C.ANGLE_WARP)
    np.random.seed(5)
    got = S.sample_table(opt)
    np.random.seed(5)
    want = np.array([[np.random.uniform(0, 6.2832), np.random.uniform(-2.6, 2.6), np.random.uniform(-2.6, 2.6)] for _ in range(9)])
    assert np.array_equal(got, want)
    np.random.seed(5)
    assert np.array_equal(E.sampler_table(opt), want)


@pytest.mark.parametrize("sampler", ["uniform", "grid"])
def test_grid_tables(sampler):
    one = S.sample_table(_opt(sampler, 24, C.ANGLE_ONLY))
    assert np.array_equal(one[:, 0], np.arange(0, 6.2832, 6.2832 / 24)) and one.shape == (24, 1)
    opt = _opt(sampler, 7, C.VEL_ONLY)
    np.random.seed(8)
    got = S.sample_table(opt)
    np.random.seed(8)
    axis = np.arange(-1.0, 1.0, 2.0 / 7)
    want = np.array([[axis[np.random.randint(len(axis))], axis[np.random.randint(len(axis))]] for _ in range(7)])
    assert np.array_equal(got, want)
    np.random.seed(8)
    assert np.array_equal(E.sampler_table(opt), want)


def test_unfold_table():
    for name in ("p8_k67", "angle", "anglemagn", "nowarp", "angle_grid1"):
        c = C.CASES[name]
        t = C.hypotheses(name)
        got = S.unfold_table(c["gml"], list(c["params"]), t)
        assert np.array_equal(got, E.unfold(c["gml"], list(c["params"]), t)) and got.shape == (c["k"], 4)
    t = C.hypotheses("anglemagn")
    got = S.unfold_table(C.CASES["anglemagn"]["gml"], list(C.VEL_ANGLEMAGN), t)
    assert np.array_equal(got[:, 2], t[:, 3] * np.sin(t[:, 2])) and np.array_equal(got[:, 3], t[:, 3] * np.cos(t[:, 2]))
    assert np.all(S.unfold_table(C.CASES["nowarp"]["gml"], list(C.VEL_ONLY), C.hypotheses("nowarp"))[:, 2:] == 0)
    with pytest.raises(ValueError):
        S.unfold_table(C.CASES["angle"]["gml"], list(C.ANGLE_WARP), np.zeros((4, 2)))


# ------------------------------------------------------------------ construction, refusals, registration
def _make(name, cls=None, **changes):
    c = C.CASES[name]
    cfg = C.solver_config(name)
    for path, v in changes.items():
        d = cfg
        keys = path.split("__")
        for k in keys[:-1]:
            d = d[k]
        if v is KeyError:
            del d[keys[-1]]
        else:
            d[keys[-1]] = v
    cls = cls or (GenerativePatchIndependent if c["kind"] == "patch" else GenerativeGlobal)
    return cls(c["shape"], c["shape"], {}, cfg)


def test_construction_and_geometry():
    s = _make("p5s3_we")
    assert s.patch_image_size == (16, 21) and s.n_patch == 336 and s._eklt_box_bound == (5, 5)
    assert np.array_equal(s._eklt_boxes, boxes_of("p5s3_we"))
    g = _make("global_roi")
    assert g.n_patch == 1 and np.array_equal(g._eklt_boxes, [[4, 44, 8, 60]]) and g._eklt_box_bound == (40, 52)
    assert len(s.estimate_indices) == 0 and s.best_params is None


def test_refusals():
    with pytest.raises(NotImplementedError, match="TPE"):
        _make("p8_k67", optimizer__sampler="TPE")
    with pytest.raises(NotImplementedError, match="image_gradient"):
        _make("p8_k67", cost_with_weight={"diff_norm": 1.0, "image_gradient": 0.5})
    with pytest.raises(NotImplementedError, match="scipy and torch"):
        _make("p8_k67", optimizer__method="Adam")
    with pytest.raises(NotImplementedError, match="scipy and torch"):
        _make("global_roi", optimizer__method="BFGS")
    with pytest.raises(ValueError, match="p_y"):
        _make("p8_k67", optimizer__parameters__p_y=KeyError)
    with pytest.raises(ValueError, match="angle"):
        _make("angle", optimizer__parameters__angle=KeyError)
    with pytest.raises(ValueError, match="p_magn"):
        _make("anglemagn", optimizer__parameters__p_magn=KeyError)
    with pytest.raises(ValueError, match="n_iter"):
        _make("p8_k67", optimizer__n_iter=0)
    with pytest.raises(ValueError, match="patch_size"):
        _make("p8_k67", patch_eklt={})
    s = _make("p8_k67")
    with pytest.raises(ValueError, match="route"):
        s.sweep(np.zeros((3, 4)), C.hypotheses("p8_k67"), frame=np.zeros(C.S), route="lds")
    with pytest.raises(ValueError, match="hypotheses"):
        s.sweep(np.zeros((3, 4)), np.zeros((5, 3)), frame=np.zeros(C.S))


def test_registration_into_a_stand_in_module():
    from event_based_bos_amd.solver import SolverBase

    class Base(SolverBase):
        pass

    reg = types.SimpleNamespace(SolverBase=Base, collections={"patch_eklt_pyramid2": object})
    patch, glob = register_eklt_into(reg)
    assert reg.collections["patch_eklt"] is patch and reg.collections["generative_max_likelihood"] is glob
    assert reg.collections["patch_eklt_pyramid2"] is object
    assert issubclass(patch, Base) and issubclass(glob, Base)
    c = C.CASES["p8_k67"]
    s = reg.collections["patch_eklt"](c["shape"], c["shape"], {}, C.solver_config("p8_k67"), None)
    assert s.n_patch == 48
    reg2 = types.SimpleNamespace(SolverBase=Base, collections={})
    register_eklt_into(reg2, names=("a", "b"))
    assert sorted(reg2.collections) == ["a", "b"]


# ------------------------------------------------------------------ the C ABI's host-only entries
@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


def test_halo_and_fit_queries(lib):
    for name in ("p8_k67", "angle", "anglemagn", "nowarp"):
        c = C.CASES[name]
        hyp4 = np.ascontiguousarray(E.unfold(c["gml"], list(c["params"]), C.hypotheses(name)))
        shifts = [shift_and_weights(px, py)[:2] for px, py in hyp4[:, 2:]]
        assert lib.ebos_eklt_sweep_halo(hyp4.ctypes.data, len(hyp4)) == max(max(abs(a), abs(b)) for a, b in shifts) + 1
    hyp4 = np.ascontiguousarray(E.unfold(C.CASES["p8_k67"]["gml"], list(C.VEL_WARP), C.hypotheses("p8_k67")))
    assert lib.ebos_eklt_sweep_halo(hyp4.ctypes.data, len(hyp4)) == 4     # |p| = 2.6: shifts -3 .. 2
    assert lib.ebos_eklt_sweep_halo(None, 3) == 0
    lds = lambda ph, pw, h: 8 * (2 * (ph + 2 * h) * (pw + 2 * h) + 2 * ph * pw)
    bound = 160 * 1024 - 4096
    for ph, pw, h in ((8, 8, 4), (5, 5, 1), (64, 64, 4), (40, 52, 4), (96, 96, 1), (128, 160, 1), (70, 70, 1), (71, 70, 1)):
        assert bool(lib.ebos_eklt_sweep_fits(ph, pw, h)) == (lds(ph, pw, h) <= bound), (ph, pw, h)
    assert lib.ebos_eklt_sweep_fits(64, 64, 4) and not lib.ebos_eklt_sweep_fits(96, 96, 1) and not lib.ebos_eklt_sweep_fits(0, 8, 1)
    patch, roi = lib.ebos_eklt_sweep_scratch_bytes(2, 48, 67, 1), lib.ebos_eklt_sweep_scratch_bytes(2, 48, 67, 2)
    assert 0 < patch < roi == lib.ebos_eklt_sweep_scratch_bytes(2, 48, 67, 0)
    assert lib.ebos_eklt_sweep_scratch_bytes(0, 48, 67, 0) == 0


def test_entries_refuse_before_any_launch(lib):
    assert lib.ebos_eklt_sweep_batch_f64(0, 48, 64, None, None, 0, None, None, None, 1, 8, 8, None, None, 1, 0, 1.0, 0, None, None, None,
                                         None, 0, None) == -1
    assert b"ebos_eklt_sweep_batch_f64" in lib.ebos_last_error()
    assert lib.ebos_eklt_sweep_batch_f64(1, 48, 64, None, None, 0, None, None, None, 1, 8, 8, None, None, 1, 0, 1.0, 0, None, None, None,
                                         None, 0, None) == -1
    assert b"NULL buffer" in lib.ebos_last_error()
    assert lib.ebos_eklt_patch_flow_batch_f64(1, 48, 64, 8, 8, 5, 8, None, None, 1, None, None, None) == -1
    assert b"patch grid" in lib.ebos_last_error()
