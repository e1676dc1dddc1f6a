"""The window axis of the generative solvers without a GPU: ``estimate_batch`` on every class that carries it, its argument errors
(raised before any GPU work), the batched C ABI in the header and the ctypes table, and the RandomState contract of the host side:
with stubs in place of the native calls, ``estimate_batch`` of three windows draws what three ``estimate`` calls draw.
``estimate`` is a batch of one window on the same driver: what it publishes and what it leaves alone, the entries it calls, its
argument errors and the order of its draws and of the "no patch selected" error are checked here as well.
"""
import contextlib
import ctypes
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_cases as C  # noqa: E402
import _gml_dep_cases as CD  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SYMBOLS = ("ebos_gml_scratch_bytes_batch", "ebos_gml_prepare_batch_f64", "ebos_gml_normalize_batch_f64",
                 "ebos_gml_solve_scale_batch_f64", "ebos_gml_dep_scratch_bytes_batch", "ebos_gml_dep_select_batch",
                 "ebos_gml_dep_init_batch_f64", "ebos_gml_dep_solve_batch_f64")


def _classes():
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver import generative as G, generative_dependent as GD

    mod = types.SimpleNamespace(SolverBase=ebos.solver.SolverBase, collections={})
    return {"pyramid": (G.GenerativePatchPyramid, C), "dependent": (GD.GenerativePatchDependent, CD),
            "pyramid_registered": (G.register_generative_into(mod), C), "dependent_registered": (GD.register_dependent_into(mod), CD)}


def _make(kind, name="yaml_128", **gml):
    cls, cases = _classes()[kind]
    c = cases.CASES[name]
    return cls(c["shape"], c["shape"], {}, cases.solver_config(name, **gml)), cases


@pytest.mark.parametrize("kind", ["pyramid", "dependent", "pyramid_registered", "dependent_registered"])
def test_estimate_batch_signature(kind):
    cls, _ = _classes()[kind]
    sig = inspect.signature(cls.estimate_batch)
    assert list(sig.parameters) == ["self", "windows", "frames", "background", "max_batch"]
    assert all(sig.parameters[k].default is None for k in ("frames", "background", "max_batch"))


@pytest.mark.parametrize("kind", ["pyramid", "dependent"])
def test_argument_errors_come_before_gpu_work(kind, monkeypatch):
    from event_based_bos_amd import _hip
    from event_based_bos_amd.solver import generative as G, generative_dependent as GD

    def no_gpu(*a, **k):
        raise AssertionError("GPU work before the argument checks")

    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    monkeypatch.setattr(G, "to_gpu", no_gpu)
    monkeypatch.setattr(GD, "to_gpu", no_gpu)
    s, cases = _make(kind)
    frame, ev = cases.case_inputs("yaml_128")
    with pytest.raises(ValueError, match="2 frames for 3 windows"):
        s.estimate_batch([ev, ev, ev], frames=[frame, frame])
    with pytest.raises(ValueError, match="frame shape"):
        s.estimate_batch([ev, ev], frames=[frame, frame[:-1]])
    with pytest.raises(ValueError, match="frame shape"):
        s.estimate_batch([ev, ev], frames=frame[:, :-2])
    with pytest.raises(ValueError, match="needs frame="):
        s.estimate_batch([ev, ev])
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_batch"):
            s.estimate_batch([ev, ev], frames=frame, max_batch=bad)
    b, _ = _make(kind, model_image="background")
    with pytest.raises(ValueError, match="needs background="):
        b.estimate_batch([ev, ev])
    # no window: an empty result, no GPU work, no state touched
    out = s.estimate_batch([], frames=[])
    assert out.shape == (0, 2) + tuple(cases.CASES["yaml_128"]["shape"]) and out.dtype == np.float64
    assert s.iter_cnt == 0 and s.histories == []


def test_batch_symbols_declared_and_bound():
    from event_based_bos_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebos_hip.h")).read(), flags=re.S)
    for name in BATCH_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/ebos_hip.h"
        assert name in _hip.SIGNATURES, f"{name} is not bound in _hip.py"


class _StubLib(object):
    """The native calls as no-ops on host memory; the selection writes ``n_sel + window index`` into every count, or ``counts``
    where they are given."""

    def __init__(self, n_sel, counts=None):
        self.n_sel, self.counts, self.calls = n_sel, counts, []

    def __getattr__(self, name):
        if not name.startswith("ebos_"):
            raise AttributeError(name)

        def call(*a):
            self.calls.append(name)
            if "scratch_bytes" in name:
                return 256 * (a[-1] if name.endswith("_batch") else 1)
            if name == "ebos_gml_dep_select":
                ctypes.c_int32.from_address(a[13]).value = self.n_sel
            if name == "ebos_gml_dep_select_batch":
                for b in range(a[0]):
                    ctypes.c_int32.from_address(a[15] + 4 * b).value = self.counts[b] if self.counts else self.n_sel + b
            return 0

        return call


def _stub(monkeypatch, lib):
    from event_based_bos_amd import _hip
    from event_based_bos_amd.solver import generative as G, generative_dependent as GD

    def to_cpu(x, device=None, dtype=None):
        return torch.as_tensor(np.asarray(x), dtype=dtype or torch.float64)

    monkeypatch.setattr(_hip, "require_gpu", lambda: lib)
    monkeypatch.setattr(_hip, "on_device", lambda dev: contextlib.nullcontext())
    for m in (G, GD):
        monkeypatch.setattr(m, "to_gpu", to_cpu)
        monkeypatch.setattr(m, "stream_ptr", lambda dev=None: None)


@pytest.mark.parametrize("kind", ["pyramid", "dependent"])
def test_random_state_contract_on_the_host(kind, monkeypatch):
    s, cases = _make(kind)
    H, W = cases.CASES["yaml_128"]["shape"]
    monkeypatch.setattr(type(s._gml_imager), "_accumulate", lambda self, *a, **k: torch.zeros(1, 2, H, W, dtype=torch.float64))
    frame, ev = cases.case_inputs("yaml_128")
    windows = [ev[:100], ev[:50], ev[:75]]

    # the sequential stub selects n_sel + i patches in window i, as the batched one does
    lib = _StubLib(7)
    _stub(monkeypatch, lib)
    np.random.seed(5)
    for i, w in enumerate(windows):
        lib.n_sel = 7 + i
        s.estimate(w, frame=frame)
    after_sequential = np.random.get_state()
    assert s.iter_cnt == 3

    t, _ = _make(kind)
    lib = _StubLib(7)
    _stub(monkeypatch, lib)
    np.random.seed(5)
    out = t.estimate_batch(windows, frames=frame)
    after_batch = np.random.get_state()
    assert out.shape == (3, 2, H, W) and t.iter_cnt == 3 and len(t.histories) == 3
    assert after_batch[0] == after_sequential[0] and after_batch[2:] == after_sequential[2:]
    assert np.array_equal(after_batch[1], after_sequential[1])
    assert np.random.random() != 0.0
    # a batch issues one window's launches: one solve call per scale (pyramid) or one in all (dependent)
    solves = [c for c in lib.calls if "solve" in c]
    assert solves == (["ebos_gml_solve_scale_batch_f64"] * 4 if kind == "pyramid" else ["ebos_gml_dep_solve_batch_f64"])
    if kind == "dependent":
        assert lib.calls.count("ebos_gml_dep_select_batch") == 1


def _stubbed(kind, monkeypatch, lib):
    s, cases = _make(kind)
    H, W = cases.CASES["yaml_128"]["shape"]
    monkeypatch.setattr(type(s._gml_imager), "_accumulate", lambda self, *a, **k: torch.zeros(1, 2, H, W, dtype=torch.float64))
    _stub(monkeypatch, lib)
    return s, cases.case_inputs("yaml_128")


@pytest.mark.parametrize("kind", ["pyramid", "dependent"])
def test_estimate_is_a_batch_of_one_and_leaves_the_lists(kind, monkeypatch):
    lib = _StubLib(7)
    s, (frame, ev) = _stubbed(kind, monkeypatch, lib)
    lists = ("histories",) + (("params_per_scale_batch",) if kind == "pyramid" else ("params_batch", "estimate_indices_batch"))
    np.random.seed(5)
    s.estimate_batch([ev[:100], ev[:50], ev[:75]], frames=frame)
    assert s.iter_cnt == 3 and all(len(getattr(s, k)) == 3 for k in lists)
    before = {k: list(getattr(s, k)) for k in lists}
    s.cost_func.history["loss"] = ["stale"]
    del lib.calls[:]
    out = s.estimate(ev[:60], frame=frame)
    assert out.shape == (2,) + tuple(frame.shape) and out.dtype == np.float64
    for k in lists:   # the same objects, in the same order
        assert len(getattr(s, k)) == 3 and all(a is b for a, b in zip(getattr(s, k), before[k]))
    n_rows = s._gml_n_iter if kind == "dependent" else sum(s._gml_n_iter // (5 - i + 1) for i in range(1, 5))
    hist = s.cost_func.get_history()
    assert "stale" not in hist["loss"] and all(len(v) == n_rows for v in hist.values())
    assert s.iter_cnt == 4
    native = [c for c in lib.calls if any(w in c for w in ("prepare", "normalize", "select", "init", "solve"))]
    assert native and all("_batch" in c for c in native), native
    assert [c for c in native if "solve" in c] == (["ebos_gml_solve_scale_batch_f64"] * 4 if kind == "pyramid" else
                                                   ["ebos_gml_dep_solve_batch_f64"])


def test_no_patch_selected_in_window_order(monkeypatch):
    """Window 0 selects three patches and draws, window 1 selects none: ``estimate`` and ``estimate_batch`` raise the same error
    there and leave numpy's global RandomState in the same state."""
    states, errors = [], []
    for batched in (False, True):
        lib = _StubLib(0, counts=[3, 0])
        s, (frame, ev) = _stubbed("dependent", monkeypatch, lib)
        np.random.seed(5)
        with pytest.raises(ValueError, match="no patch selected") as err:
            if batched:
                s.estimate_batch([ev[:100], ev[:50]], frames=frame)
            else:
                s.estimate(ev[:100], frame=frame)
                lib.counts = [0]
                s.estimate(ev[:50], frame=frame)
        errors.append(str(err.value))
        states.append(np.random.get_state())
        assert s.iter_cnt == (0 if batched else 1)
    assert errors[0] == errors[1]
    assert states[0][0] == states[1][0] and states[0][2:] == states[1][2:] and np.array_equal(states[0][1], states[1][1])
    np.random.seed(5)
    np.random.random(4)   # the discarded draw and window 0's three
    assert np.array_equal(np.random.get_state()[1], states[0][1]) and np.random.get_state()[2] == states[0][2]
    # no window selects a patch: nothing is drawn, by either entry
    for batched in (False, True):
        s, (frame, ev) = _stubbed("dependent", monkeypatch, _StubLib(0, counts=[0, 0]))
        np.random.seed(5)
        start = np.random.get_state()
        with pytest.raises(ValueError, match="no patch selected"):
            s.estimate_batch([ev[:100], ev[:50]], frames=frame) if batched else s.estimate(ev[:100], frame=frame)
        assert np.array_equal(np.random.get_state()[1], start[1]) and np.random.get_state()[2] == start[2]


@pytest.mark.parametrize("kind", ["pyramid", "dependent"])
def test_estimate_argument_errors_come_before_gpu_work(kind, monkeypatch):
    from event_based_bos_amd import _hip
    from event_based_bos_amd.solver import generative as G, generative_dependent as GD

    def no_gpu(*a, **k):
        raise AssertionError("GPU work before the argument checks")

    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    monkeypatch.setattr(G, "to_gpu", no_gpu)
    monkeypatch.setattr(GD, "to_gpu", no_gpu)
    s, cases = _make(kind)
    frame, ev = cases.case_inputs("yaml_128")
    who = "generative dependent solver: " if kind == "dependent" else "generative solver: "
    with pytest.raises(ValueError, match="needs frame=") as err:
        s.estimate(ev)
    assert str(err.value).startswith(who)
    for bad in (frame[:-1], frame[:, :-2], frame[None]):
        with pytest.raises(ValueError, match="frame shape") as err:
            s.estimate(ev, frame=bad)
        assert str(err.value).startswith(who)
    assert s._gml_frame is None and s.iter_cnt == 0
    b, _ = _make(kind, model_image="background")
    with pytest.raises(ValueError, match="needs background=") as err:
        b.estimate(ev)
    assert str(err.value).startswith(who)
    with pytest.raises(ValueError, match="frame shape"):
        b.estimate(ev, background=frame[:-1])
    assert b._gml_frame is None and b.iter_cnt == 0
