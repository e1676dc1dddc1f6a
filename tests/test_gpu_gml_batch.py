"""``estimate_batch`` of the generative solvers on the GPU (csrc/gml.hip ``ebos_gml_*_batch*``): several windows per launch.

``estimate`` is the batch driver at one window; tests/test_gpu_gml.py and tests/test_gpu_gml_dep.py pin it, and with it the driver
at B = 1, to the reference's golden_gml.npz / golden_gml_dep.npz and to the torch restatement.  This file compares the driver at
B > 1 (and ``estimate_batch`` at B = 1) with that: ``estimate_batch`` is defined as equal to ``estimate`` on the windows in order,
and a batched pass runs the single-window body on the view of its window, so everything is compared with ``np.array_equal``: no
tolerance, no excluded case.  ``n_iter`` is shortened (two runs of this package are compared, so the
fixture's length is not needed).  Two cases go through ``estimate_batch`` against the fixture itself, with the existing bounds.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_cases as CP  # noqa: E402
import _gml_dep_cases as CD  # noqa: E402
from test_gml_dep import BOUNDS  # noqa: E402
from test_gpu_gml import STABLE  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_P = np.load(os.path.join(HERE, "golden", "golden_gml.npz"))
GOLDEN_D = np.load(os.path.join(HERE, "golden", "golden_gml_dep.npz"))
N_ITER = 36   # pyramid: 9, 12, 18, 36 iterations at the four scales
N_WIN = 5
KINDS = {"pyramid": ("generative_patch_pyramid", CP), "dependent": ("generative_patch_dependent", CD)}
PYRAMID_CASES = ["yaml_128", "yaml_128_roi", "nowarp_128", "nopol_128", "evhist_128", "sigma0_log_128", "yaml_260", "terms_260"]
DEPENDENT_CASES = ["yaml_128", "yaml_128_roi", "nowarp_128", "vel_128", "vel_nowarp_128", "thres_128", "nopol_128", "evhist_128",
                   "odd_128", "yaml_260"]
ALL = [("pyramid", n) for n in PYRAMID_CASES] + [("dependent", n) for n in DEPENDENT_CASES]


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as ebos
    return ebos


def _solver(ebos, kind, name, n_iter=N_ITER, **gml):
    key, cases = KINDS[kind]
    c = cases.CASES[name]
    cfg = cases.solver_config(name, **gml)
    if n_iter is not None:
        cfg["optimizer"]["n_iter"] = n_iter
    return ebos.solver.collections[key](c["shape"], c["shape"], {}, cfg)


def _windows(kind, name, n=N_WIN):
    """-> (frame, n windows over it): different event seeds, different event counts; window 0 is the case's own."""
    cases = KINDS[kind][1]
    c = cases.CASES[name]
    H, W = c["shape"]
    frame, ev0 = cases.case_inputs(name)
    make = CD.clustered_events if c.get("clustered") else CP.synth_events
    return frame, [ev0] + [make(int(c["n_events"] * (1.0 - 0.17 * i)) + 13 * i, H, W, 900 + 31 * i + c["seed"]) for i in range(1, n)]


def _result(kind, s, flow, history):
    """Everything a window leaves behind, as arrays."""
    out = {"flow": flow}
    out.update({"hist_" + k: np.array(v) for k, v in history.items()})
    return out


def _sequential(ebos, kind, name, frame, windows, seed, **gml):
    s = _solver(ebos, kind, name, **gml)
    np.random.seed(seed)
    res = []
    for ev in windows:
        flow = s.estimate(ev, frame=frame, background=frame)
        r = _result(kind, s, flow, s.cost_func.get_history())
        if kind == "pyramid":
            r.update({f"x{k}": v for k, v in s.params_per_scale.items()})
        else:
            r.update({"x": s.params, "sel": s.estimate_indices})
        res.append(r)
    return s, res, np.random.get_state()


def _batched(ebos, kind, name, frames, windows, seed, max_batch=None, **gml):
    s = _solver(ebos, kind, name, **gml)
    np.random.seed(seed)
    flows = s.estimate_batch(windows, frames=frames, background=frames if not isinstance(frames, list) else frames[0],
                             max_batch=max_batch)
    res = []
    for i in range(len(windows)):
        r = _result(kind, s, flows[i], s.histories[i])
        if kind == "pyramid":
            r.update({f"x{k}": v for k, v in s.params_per_scale_batch[i].items()})
        else:
            r.update({"x": s.params_batch[i], "sel": s.estimate_indices_batch[i]})
        res.append(r)
    return s, res, np.random.get_state()


def _assert_same(a, b, what):
    assert len(a) == len(b), what
    for i, (ra, rb) in enumerate(zip(a, b)):
        assert sorted(ra) == sorted(rb), (what, i)
        for k in ra:
            assert ra[k].shape == rb[k].shape and np.array_equal(ra[k], rb[k]), f"{what}: window {i}, {k} differs"


def _assert_state(sa, sb):
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:], "numpy's global RandomState differs"


@pytest.mark.parametrize("kind,name", ALL)
def test_batch_equals_sequential_bit_for_bit(ebos, kind, name):
    """B = 1, 2, 5 and five windows with max_batch=2, model_image current with one frame per window."""
    frame, windows = _windows(kind, name)
    seed = KINDS[kind][1].CASES[name]["init_seed"]
    runs = {b: _sequential(ebos, kind, name, frame, windows[:b], seed) for b in (1, 2, N_WIN)}
    assert len({len(w) for w in windows}) == N_WIN
    for b in (1, 2, N_WIN):
        s0, ref, st0 = runs[b]
        s, got, st = _batched(ebos, kind, name, [frame] * b, windows[:b], seed)
        _assert_same(ref, got, f"{kind} {name} B={b}")
        _assert_state(st0, st)
        # afterwards the solver holds the LAST window's values, as after sequential calls
        assert s.iter_cnt == s0.iter_cnt == b and s.cost_func.get_history() == s0.cost_func.get_history()
        if kind == "pyramid":
            assert all(np.array_equal(s.params_per_scale[k], s0.params_per_scale[k]) for k in s0.params_per_scale)
        else:
            assert np.array_equal(s.params, s0.params) and np.array_equal(s.estimate_indices, s0.estimate_indices)
    s0, ref, st0 = runs[N_WIN]
    s, got, st = _batched(ebos, kind, name, [frame] * N_WIN, windows, seed, max_batch=2)
    _assert_same(ref, got, f"{kind} {name} max_batch=2")
    _assert_state(st0, st)
    assert s.iter_cnt == N_WIN


@pytest.mark.parametrize("kind", ["pyramid", "dependent"])
@pytest.mark.parametrize("model_image", ["background", "current"])
def test_shared_model_image(ebos, kind, model_image):
    """One model image for every window (frame stride 0): ``model_image: background`` by overriding the case's option, and
    ``current`` with one frame for all."""
    name = "yaml_128_roi"
    frame, windows = _windows(kind, name)
    seed = KINDS[kind][1].CASES[name]["init_seed"]
    _, ref, st0 = _sequential(ebos, kind, name, frame, windows, seed, model_image=model_image)
    for mb in (None, 2):
        s, got, st = _batched(ebos, kind, name, frame, windows, seed, max_batch=mb, model_image=model_image)
        _assert_same(ref, got, f"{kind} {model_image} max_batch={mb}")
        _assert_state(st0, st)
    # the background is kept, as estimate keeps it: a further batch needs none
    if model_image == "background":
        np.random.seed(seed)
        again = s.estimate_batch(windows[:2])
        assert np.array_equal(again[0], ref[0]["flow"]) and np.array_equal(again[1], ref[1]["flow"])


def test_windows_with_their_own_frames(ebos):
    """model_image current with a different frame per window (frame stride H W)."""
    for kind in ("pyramid", "dependent"):
        name = "yaml_128_roi"
        frame, windows = _windows(kind, name, 3)
        H, W = frame.shape
        frames = [frame, CP.frame_image(H, W, 71), CP.frame_image(H, W, 72)]
        s0 = _solver(ebos, kind, name)
        np.random.seed(3)
        ref = [s0.estimate(ev, frame=f) for ev, f in zip(windows, frames)]
        s = _solver(ebos, kind, name)
        np.random.seed(3)
        got = s.estimate_batch(windows, frames=np.stack(frames))
        assert all(np.array_equal(a, b) for a, b in zip(ref, got)), kind
        assert not np.array_equal(got[1], got[2])


class _Draws(object):
    """``np.random.random`` served from a prepared stream, so that a window in the middle of a batch can be given the draws the
    fixture's window was made with."""

    def __init__(self, values):
        self.values, self.used = values, 0

    def __call__(self, size=None):
        n = 1 if size is None else int(size)
        out = self.values[self.used:self.used + n].copy()
        assert len(out) == n
        self.used += n
        return out[0] if size is None else out


def _fixture_batches(ebos, kind, name, monkeypatch, draws_per_window):
    """The case as window 0 and as window B - 1 of a mixed batch, at the fixture's n_iter -> [(solver, flow, index)]."""
    cases = KINDS[kind][1]
    frame, windows = _windows(kind, name, 3)
    case, others = windows[0], windows[1:]
    init = np.random.RandomState(cases.CASES[name]["init_seed"]).random_sample(draws_per_window)
    other = np.random.RandomState(4).random_sample(2 * draws_per_window)
    out = []
    for order, stream, idx in (([case] + others, np.concatenate([init, other]), 0),
                               (others + [case], np.concatenate([other, init]), 2)):
        feed = _Draws(stream)
        monkeypatch.setattr(np.random, "random", feed)
        s = _solver(ebos, kind, name, n_iter=None)
        flows = s.estimate_batch(order, frames=[frame] * 3)
        assert feed.used == 3 * draws_per_window
        out.append((s, flows[idx], idx))
    return out


def test_pyramid_fixture_through_estimate_batch(ebos, monkeypatch):
    """yaml_260 (in STABLE of tests/test_gpu_gml.py) with the assertions of its test_fixture_end_to_end: 1e-10 on the first
    iteration, 1e-9 on the whole history and the flow."""
    name = "yaml_260"
    assert name in STABLE
    H, W = CP.CASES[name]["shape"]
    per_window = 1 + (-(-H // 64)) * (-(-W // 64))   # one discarded draw, one per patch of the coarsest scale
    for s, flow, idx in _fixture_batches(ebos, "pyramid", name, monkeypatch, per_window):
        h = s.histories[idx]
        ref = GOLDEN_P[name + "_loss"]
        loss = np.array(h["loss"])
        assert loss.shape == ref.shape
        assert abs(loss[0] - ref[0]) <= 1e-10 * abs(ref[0])
        for k in CP.CASES[name]["cost"]:
            r = GOLDEN_P[f"{name}_{k}"]
            assert abs(h[k][0] - r[0]) <= 1e-10 * max(abs(r[0]), 1e-300), k
        d = np.abs(loss - ref) / np.abs(ref)
        fe = np.abs(flow[:, CP.stored_rows(name)] - GOLDEN_P[name + "_flow"]).max() / float(GOLDEN_P[name + "_flow_absmax"])
        print(f"pyramid {name} as window {idx}: first {d[0]:.1e}  max {d.max():.1e}  flow {fe:.1e}")
        assert d.max() <= 1e-9 and fe <= 1e-9
        xmin, xmax, ymin, ymax = CP.roi_of(name)
        outside = flow.copy()
        outside[:, xmin:xmax, ymin:ymax] = 0
        assert flow.shape == (2, H, W) and not outside.any()


def test_dependent_fixture_through_estimate_batch(ebos, monkeypatch):
    """yaml_260 with the assertions of tests/test_gpu_gml_dep.py::test_fixture_end_to_end and its BOUNDS (1e-9, 1e-9)."""
    name = "yaml_260"
    assert BOUNDS[name] == (1e-9, 1e-9)
    c = CD.CASES[name]
    probe = _solver(ebos, "dependent", name)
    gh, gw = probe.patch_image_size
    sel = np.unpackbits(GOLDEN_D[name + "_selected"])[:gh * gw].astype(bool)
    per_window = 1 + int(sel.sum())   # no thresholding: every window selects the ROI's patches
    for s, flow, idx in _fixture_batches(ebos, "dependent", name, monkeypatch, per_window):
        assert np.array_equal(s.estimate_indices_batch[idx], np.nonzero(sel)[0])
        h = s.histories[idx]
        ref = GOLDEN_D[name + "_loss"]
        loss = np.array(h["loss"])
        assert loss.shape == ref.shape
        assert abs(loss[0] - ref[0]) <= 1e-10 * abs(ref[0])
        for k in c["cost"]:
            assert abs(h[k][0] - GOLDEN_D[f"{name}_{k}"][0]) <= 1e-10 * max(abs(GOLDEN_D[f"{name}_{k}"][0]), 1e-300), k
        d = np.abs(loss - ref) / np.abs(ref)
        fe = np.abs(flow[:, CD.stored_rows(name)] - GOLDEN_D[name + "_flow"]).max() / float(GOLDEN_D[name + "_flow_absmax"])
        x, xr = s.params_batch[idx], GOLDEN_D[name + "_x"]
        xe = np.abs(x[:, CD.stored_param_rows(name)] - xr).max() / max(np.abs(xr).max(), 1e-300)
        print(f"dependent {name} as window {idx}: loss first {d[0]:.1e} max {d.max():.1e}  flow {fe:.1e}  x {xe:.1e}")
        hb, fb = BOUNDS[name]
        assert d.max() <= hb and fe <= fb and xe <= fb, (d.max(), fe, xe)
        assert flow.shape == (2,) + tuple(c["shape"]) and not x[:, ~sel.reshape(gh, gw)].any()


@pytest.mark.parametrize("kind,name", [("pyramid", "yaml_128_roi"), ("dependent", "thres_128")])
def test_two_batches_bit_identical_and_estimate_undisturbed(ebos, kind, name):
    frame, windows = _windows(kind, name)
    seed = KINDS[kind][1].CASES[name]["init_seed"]
    s, a, _ = _batched(ebos, kind, name, [frame] * N_WIN, windows, seed)
    _, b, _ = _batched(ebos, kind, name, [frame] * N_WIN, windows, seed)
    _assert_same(a, b, f"{kind} {name}: two batches")
    # a plain estimate after the batch, on the same solver, against a fresh solver's
    np.random.seed(11)
    after = s.estimate(windows[1], frame=frame, background=frame)
    fresh = _solver(ebos, kind, name)
    np.random.seed(11)
    alone = fresh.estimate(windows[1], frame=frame, background=frame)
    assert np.array_equal(after, alone) and s.cost_func.get_history() == fresh.cost_func.get_history()
    assert s.iter_cnt == N_WIN + 1


def test_registered_classes_carry_the_method(ebos):
    import types

    from event_based_bos_amd import solver
    reg = types.SimpleNamespace(SolverBase=solver.SolverBase, collections={})
    solver.register_dependent_into(reg)
    frame, windows = _windows("dependent", "yaml_128_roi", 2)
    cfg = CD.solver_config("yaml_128_roi")
    cfg["optimizer"]["n_iter"] = 8
    shape = CD.CASES["yaml_128_roi"]["shape"]
    s = reg.collections["patch_eklt_dependent"](shape, shape, {}, cfg)
    np.random.seed(1)
    got = s.estimate_batch(windows, frames=frame)
    t = _solver(ebos, "dependent", "yaml_128_roi", n_iter=8)
    np.random.seed(1)
    assert np.array_equal(got[1], [t.estimate(w, frame=frame) for w in windows][1])
