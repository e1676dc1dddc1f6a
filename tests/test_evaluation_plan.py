"""CPU checks of the evaluation plan (event_based_bos_amd/evaluation.py): ``plan_evaluation`` against the restated index loop of
the reference driver (tests/_evaluation_ref.py), field by field, and the text writer's lines."""
import copy
import dataclasses

import numpy as np
import pytest

from _evaluation_ref import FakeEvents, FakeFrames, reference_line, reference_steps
from event_based_bos_amd.evaluation import EvalStep, flow_error_statistics, plan_evaluation
from event_based_bos_amd.solver.base import SolverBase

SHAPE = (20, 30)


def _stores(n_frames=24, period=0.008, n_events=6000, seed=0, shapes=SHAPE):
    rs = np.random.RandomState(seed)
    stamps = 0.1 + period * np.arange(n_frames) + rs.uniform(0, 1e-4, n_frames)
    # event times: dense in the middle of the recording, sparse at both ends, a few before the first and after the last frame
    t = np.sort(np.concatenate([rs.uniform(0.09, stamps[-1] + 0.01, n_events // 10),
                                rs.uniform(stamps[6], stamps[14], n_events)]))
    t = np.round(t * 1e6) / 1e6
    return FakeEvents(t), FakeFrames(stamps, shapes), stamps


def _config(dt=1, time_list=None, n_events=None, max_time=None, crop=(20, 20), common=None):
    cfg = {"evaluation": {"dt": dt, "time_list": time_list},
           "common_params": common or {"xmin": 0, "xmax": 20, "ymin": 5, "ymax": 25},
           "data": {"crop_height": crop[0], "crop_width": crop[1], "height": SHAPE[0], "width": SHAPE[1]}}
    if n_events is not None:
        cfg["data"]["n_events_per_batch"] = n_events
    if max_time is not None:
        cfg["data"]["max_time_per_event_batch"] = max_time
    return cfg


def _cases():
    ev, fr, st = _stores()
    whole = [[st[0] - 0.001, st[-1] + 0.001]]
    two = [[st[1] + 1e-4, st[8] + 1e-4], [st[12] + 1e-4, st[22] + 1e-4]]
    return {
        "dt1": _config(1, whole),
        "dt3": _config(3, whole),
        "two_intervals_dt3": _config(3, two),
        "few_events_widen_past_both_ends": _config(1, whole, n_events=20000),   # more than the recording holds: runs past 0 and len
        "few_events_widen": _config(1, whole, n_events=300),
        "too_many_events": _config(1, [[st[6], st[15]]], n_events=50),
        "max_time_cut": _config(3, whole, max_time=0.005),
        "max_time_and_n_events": _config(3, two, n_events=400, max_time=0.005),
        "both_absent_two_intervals": _config(1, two),
        "interval_too_short": _config(3, [[st[4] + 1e-4, st[6] + 1e-4]]),
        "short_then_long": _config(1, [[st[4] + 1e-4, st[5] + 2e-4], [st[10], st[16]]]),
        "wrong_crop_all_skipped": _config(1, whole, crop=(20, 22)),
    }


CASES = _cases()


def _as_dict(step: EvalStep) -> dict:
    return dataclasses.asdict(step)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_reference_loop(name):
    ev, fr, _ = _stores()
    cfg = CASES[name]
    want = reference_steps(copy.deepcopy(cfg), ev, fr)
    got = plan_evaluation(copy.deepcopy(cfg), ev, fr)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        gd = _as_dict(g)
        assert set(gd) == set(w)
        for k in w:
            assert type(gd[k]) == type(w[k]) or isinstance(gd[k], (float, np.floating)), (name, k)
            assert gd[k] == w[k], (name, k, gd[k], w[k])


def test_the_cases_reach_what_they_are_for():
    ev, fr, st = _stores()
    n = len(ev)
    steps = {k: plan_evaluation(copy.deepcopy(c), ev, fr) for k, c in CASES.items()}
    assert len(steps["dt1"]) > 10 and all(s.i2 - s.i1 == 3 for s in steps["dt3"])
    assert steps["interval_too_short"] == []
    wide = steps["few_events_widen_past_both_ends"]
    assert all(s.est_range == (0, n) for s in wide)                              # clamped at both ends
    assert any(s.est_range[1] - s.est_range[0] == 300 - (300 - (s.gt_range[1] - s.gt_range[0])) % 2 for s in steps["few_events_widen"]
               if s.gt_range[1] - s.gt_range[0] < 300 and s.est_range[0] > 0 and s.est_range[1] < n)
    assert all(s.est_range[1] - s.est_range[0] == 50 for s in steps["too_many_events"])
    assert all(abs(s.gt_time_scale - 0.005) < 1e-12 and s.t2 < fr.timestamps[s.i2] for s in steps["max_time_cut"])
    assert all(s.est_range[1] <= s.gt_range[1] for s in steps["max_time_cut"])
    skipped = steps["wrong_crop_all_skipped"]
    assert skipped and all(not s.run and s.i_frame == 0 for s in skipped)
    assert [s.i_frame for s in steps["two_intervals_dt3"]] == list(range(len(steps["two_intervals_dt3"])))   # counts across intervals


def test_a_skipped_pair_does_not_advance_i_frame():
    """Frames of two sizes: the pairs that touch a small frame are skipped and not counted."""
    shapes = [SHAPE] * 24
    shapes[9] = (20, 18)
    ev, fr, st = _stores(shapes=shapes)
    cfg = _config(2, [[st[0] - 0.001, st[-1] + 0.001]])
    want = reference_steps(copy.deepcopy(cfg), ev, fr)
    got = plan_evaluation(copy.deepcopy(cfg), ev, fr)
    assert [_as_dict(g) for g in got] == want
    off = [s for s in got if not s.run]
    assert sorted((s.i1, s.i2) for s in off) == [(7, 9), (9, 11)]
    ran = [s for s in got if s.run]
    assert [s.i_frame for s in ran] == list(range(len(ran)))


def test_text_lines(tmp_path):
    """``save_flow_error_as_text`` under the evaluator's file names: ``frame <i>::{...}`` lines a literal reader parses."""
    import ast

    from event_based_bos_amd import evaluation

    class Viz(object):
        save_dir = str(tmp_path)

    s = SolverBase(SHAPE, (20, 20), None, {}, Viz())
    ev, fr, st = _stores()
    steps = plan_evaluation(copy.deepcopy(CASES["max_time_cut"]), ev, fr)[:3]
    rs = np.random.RandomState(1)
    want = {evaluation.TEXT_WITHOUT_MASK: "", evaluation.TEXT_WITH_MASK: "", evaluation.TEXT_TIMESTAMPS: ""}
    dicts = []
    for step in steps:
        e0 = {k: np.float64(rs.rand()) for k in ("EPE", "1PE", "2PE", "3PE", "5PE", "10PE", "20PE", "AE")}
        e1 = {k: np.float64(rs.rand()) for k in e0}
        ts = {"t1": step.t1, "t2": step.t2}
        dicts.append(e0)
        for name, d in ((evaluation.TEXT_WITHOUT_MASK, e0), (evaluation.TEXT_WITH_MASK, e1), (evaluation.TEXT_TIMESTAMPS, ts)):
            s.save_flow_error_as_text(step.i_frame, d, name)
            want[name] += reference_line(step.i_frame, d)
    for name, text in want.items():
        got = open(tmp_path / name).read()
        assert got == text
        for line in got.splitlines():
            ast.literal_eval(line[line.find("::") + 2:])
    assert sorted(s.evaluation_text_list) == sorted(str(tmp_path / n) for n in (evaluation.TEXT_WITHOUT_MASK, evaluation.TEXT_WITH_MASK))
    stats = flow_error_statistics(dicts)
    epe = np.array([d["EPE"] for d in dicts])
    assert stats["EPE"]["mean"] == np.mean(epe) and stats["EPE"]["n_data"] == 3 and stats["EPE"]["max"] == epe.max()
    assert stats["1PE"]["mean"] == np.mean(np.array([d["1PE"] for d in dicts]) * 100.0)
