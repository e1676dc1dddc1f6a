"""The sampled EKLT solvers on the GPU (csrc/eklt_sweep.hip ebos_eklt_*, event_based_bos_amd.solver.eklt_sweep) against the plain
numpy restatement tests/_eklt_ref.py (itself pinned to the reference by tests/test_eklt.py) and the reference's fixture
golden_eklt.npz.

The bar.  A cost is the largest of a box's column sums of |P - Q|.  The kernel's float64 sums run in another order than numpy's,
so a column sum may differ by the forward-error bound of a sum of n terms in any order, n 2^-52 sum |terms|; with n = n_box (the
norms under P and Q are sums over the whole box) and sum |P| + sum |Q| over the column for the terms, the restatement computes
``bar = n_box 2^-52 max_c (sum_r |P| + sum_r |Q|)`` from its own P and Q, and the tests allow 4 bar: the column sum itself, the two
norms that scale its terms, and the histogram's scale (the prepare pass leaves q divided by the whole image's norm, which Q's own
normalisation takes out again up to rounding).  Winners must equal the restatement's wherever its best leads its runner-up by
more than twice that; elsewhere either of the two may win, for at most 1 % of the scored boxes.
"""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eklt_cases as C  # noqa: E402
import _eklt_ref as E  # noqa: E402
import _gml_dep_ref as D  # noqa: E402
from test_eklt import GOLDEN, INPLACE, boxes_of, restated_table, zero_norm_index  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_FACTOR = 4.0
ESCAPE_SHARE = 0.01
WORST = {}


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as ebos
    return ebos


def _solver(ebos, name):
    c = C.CASES[name]
    key = "generative_patch_independent" if c["kind"] == "patch" else "generative_global"
    return ebos.solver.collections[key](c["shape"], c["shape"], {}, C.solver_config(name))


_SWEEPS = {}


def _sweep(ebos, name, route=None):
    """(cost, best_index, selected) of the case's explicit table on the GPU, computed once per (case, route) and shared."""
    if (name, route) not in _SWEEPS:
        frame, events = C.case_inputs(name)
        out = _solver(ebos, name).sweep(events, C.hypotheses(name), frame=frame, background=frame, route=route)
        for a in out:
            a.setflags(write=False)
        _SWEEPS[(name, route)] = out
    return _SWEEPS[(name, route)]


def _selection(name):
    """The boxes ``estimate`` would score: centre inside the crop and, with thresholding, enough events (tests/_gml_dep_ref.py)."""
    c = C.CASES[name]
    n = len(boxes_of(name))
    if c["kind"] == "global":
        return np.ones(n, dtype=bool)
    pe = c["patch"]
    sel = np.zeros(n, dtype=bool)
    sel[D.select(C.case_inputs(name)[1], *c["shape"], pe["patch_size"], pe["sliding_window"], C.roi_of(name), pe["do_event_thresholding"],
                 pe["event_thres"])] = True
    return sel


def _check_table(name, cost, best, selected, factor=BAR_FACTOR):
    """cost [P, K] against the restatement within factor x bar; winners; -> the worst observed fraction of the bar."""
    want, ok, bar, _ = restated_table(name, inplace=False)
    ok = ok & _selection(name)   # (the restated table scores every box, as the fixture's does)
    assert np.array_equal(selected, ok)
    assert not np.isnan(cost[ok]).any(), "a scored box's cost row is fully written"
    assert np.isnan(cost[~ok]).all(), "an unscored box's cost row is untouched"
    frac = np.abs(cost[ok] - want[ok]) / bar[ok]
    print(f"{name}: worst |gpu - numpy| = {frac.max():.3f} bar ({np.abs(cost[ok] - want[ok]).max():.2e}), allowed {factor}")
    assert frac.max() <= factor
    # best_index is the row argmin of the stored cost, the lowest index first
    assert np.array_equal(best, E.argmin_rows(cost))
    # winners: the restatement's, unless its best leads its runner-up by no more than twice the allowed difference
    ref_best = E.argmin_rows(want)
    K = want.shape[1]
    escaped = 0
    for i in np.nonzero(ok)[0]:
        if best[i] == ref_best[i]:
            continue
        order = np.argsort(want[i], kind="stable")
        lead = want[i, order[1]] - want[i, order[0]] if K > 1 else np.inf
        assert lead <= 2 * factor * bar[i].max() and best[i] in order[:2], (name, i, best[i], ref_best[i], lead)
        escaped += 1
    share = escaped / max(int(ok.sum()), 1)
    print(f"{name}: {escaped} of {int(ok.sum())} winners on a near-tie ({100 * share:.2f} %)")
    assert share <= ESCAPE_SHARE
    return float(frac.max())


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_sweep_cost_table(ebos, name):
    cost, best, selected = _sweep(ebos, name)
    WORST[name] = _check_table(name, cost, best, selected)
    z = zero_norm_index(name)
    if z is not None:
        assert not selected[z] and best[z] == -1
    if name == "thres":
        assert 0 < selected.sum() < len(selected) // 4


def test_unwarped_and_special_rows_are_in_the_table():
    """The table of the widest case holds fractions of exactly 0 and 31/32 and every integer shift from -3 to 2."""
    from _eklt_warp64 import shift_and_weights

    hyp4 = restated_table("p8_k67")[3]
    sw = [shift_and_weights(px, py) for px, py in hyp4[:, 2:]]
    assert {s[0] for s in sw} | {s[1] for s in sw} >= {-3, -2, -1, 0, 1, 2}
    assert any(w[2] == (1.0, 0.0, 0.0, 0.0) for w in sw) and any(w[2][3] == float(np.float32(31 / 32) * np.float32(31 / 32)) for w in sw)


def test_two_runs_are_bit_identical(ebos):
    frame, events = C.case_inputs("p8_k67")
    a = _sweep(ebos, "p8_k67")
    b = _solver(ebos, "p8_k67").sweep(events, C.hypotheses("p8_k67"), frame=frame, background=frame)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def test_cost_does_not_depend_on_how_the_table_is_cut(ebos):
    frame, events = C.case_inputs("p8_k67")
    cost = _sweep(ebos, "p8_k67")[0]
    t = C.hypotheses("p8_k67")
    s = _solver(ebos, "p8_k67")
    parts = [s.sweep(events, t[lo:hi], frame=frame, background=frame)[0] for lo, hi in ((0, 30), (30, 31), (31, 67))]
    assert np.array_equal(np.concatenate(parts, axis=1), cost)


def test_patch_route_and_roi_route_agree(ebos):
    """A box both routes can take.  The patch route sums a box serially in one thread, the ROI route in strided partial sums and a
    tree: the same terms in another order, so each is within the bar of the restatement and they are within two bars of each
    other -- not bit-equal."""
    want, ok, bar, _ = restated_table("p8_k67", inplace=False)   # (no ROI, no thresholding: every box is scored)
    auto, patch, roi = (_sweep(ebos, "p8_k67", r) for r in (None, "patch", "roi"))
    assert np.array_equal(auto[0], patch[0], equal_nan=True), "8 x 8 boxes with a halo of 4 fit in LDS: auto is the patch route"
    _check_table("p8_k67", *roi)
    assert (np.abs(patch[0][ok] - roi[0][ok]) <= 2 * BAR_FACTOR * bar[ok]).all()
    # a 40 x 52 box with a halo of 4 holds 79 KB: past the 64 KiB a workgroup gets by default, within the 160 KiB of a CU
    g_auto, g_patch = _sweep(ebos, "global_roi"), _sweep(ebos, "global_roi", "patch")
    assert np.array_equal(g_auto[0], g_patch[0])
    _check_table("global_roi", *_sweep(ebos, "global_roi", "roi"))


def test_boxes_no_lds_holds_take_the_roi_route(ebos):
    """96 x 96 patches (and the 128 x 160 ROI) exceed the LDS bound at any halo: auto is the ROI route, bit for bit, whose costs
    test_sweep_cost_table holds within the bar of the restatement (another summation order than numpy's, so no bit-equality with
    it); the patch route refuses."""
    for name in ("p96_roi", "global_full"):
        a, r = _sweep(ebos, name), _sweep(ebos, name, "roi")
        assert np.array_equal(a[0], r[0]) and np.array_equal(a[1], r[1])
        frame, events = C.case_inputs(name)
        with pytest.raises(RuntimeError, match="does not fit"):
            _solver(ebos, name).sweep(events, C.hypotheses(name), frame=frame, background=frame, route="patch")


ESTIMATE_CASES = [n for n in sorted(C.CASES) if n not in INPLACE]   # (there the fixture holds the reference's in-place division)


@pytest.mark.parametrize("name", ESTIMATE_CASES)
def test_estimate_against_the_fixture(ebos, name):
    c = C.CASES[name]
    frame, events = C.case_inputs(name)
    s = _solver(ebos, name)
    np.random.seed(c["init_seed"])
    flow = s.estimate(events, frame=frame, background=frame)
    H, W = c["shape"]
    assert flow.shape == (2, H, W) and flow.dtype == np.float64
    sel = np.unpackbits(GOLDEN[name + "_selected"])[:s.n_patch].astype(bool)
    z = zero_norm_index(name)
    if z is not None:
        sel[z] = False   # the reference divides by zero there; this package leaves the box out
    assert np.array_equal(s.estimate_indices, np.nonzero(sel)[0])
    # the table of the call, as the restatement draws it
    np.random.seed(c["init_seed"])
    hyp4 = E.unfold(c["gml"], list(c["params"]), E.sampler_table(C.solver_config(name)["optimizer"]))
    want_best = GOLDEN[name + "_best"].astype(np.int64)
    won = want_best >= 0
    assert np.array_equal(s.best_params[~won], np.zeros((int((~won).sum()), 4))) and np.all(np.isinf(s.best_values[~won]))
    same = (s.best_params[won] == hyp4[want_best[won]]).all(axis=1)
    print(f"{name}: {int((~same).sum())} of {int(won.sum())} winners differ from the reference's")
    assert (~same).sum() <= ESCAPE_SHARE * won.sum()
    # the flow is the upsample of the winners the GPU found ...
    if c["kind"] == "patch":
        import torch

        p, sl = c["patch"]["patch_size"], c["patch"]["sliding_window"]
        gh, gw = D.grid_shape(H, W, p, sl)
        up = D.upsample(torch.from_numpy(s.best_params[:, :2].T.reshape(2, gh, gw).copy()), p, sl, H, W).numpy()
        assert np.abs(flow - up).max() <= 1e-14
    else:
        assert np.array_equal(flow[0], np.full((H, W), s.best_params[0, 0])) and np.array_equal(flow[1], np.full((H, W), s.best_params[0, 1]))
    # ... and, where the winners are the reference's, the reference's flow
    if same.all():
        assert np.abs(flow[:, C.stored_rows(name)] - GOLDEN[name + "_flow"]).max() <= 1e-14
        assert abs(np.abs(flow).max() - float(GOLDEN[name + "_flow_absmax"])) <= 1e-14


@pytest.mark.parametrize("name", ["p5s3_we", "thres", "global_roi"])
def test_estimate_batch_is_estimate_window_by_window(ebos, name):
    c = C.CASES[name]
    wins = [C.window_inputs(name, i) for i in range(3)]
    if name == "thres":
        wins = [(f, C.clustered_events(c["n_events"], *c["shape"], 900 + i)) for i, (f, _) in enumerate(wins)]
    one = _solver(ebos, name)
    singles, indices, values = [], [], []
    for frame, events in wins:
        np.random.seed(c["init_seed"])   # every call draws the same table
        singles.append(one.estimate(events, frame=frame, background=frame))
        indices.append(one.estimate_indices)
        values.append(one.best_values)
    for order, max_batch in (((0, 1, 2), None), ((2, 0, 1), None), ((0, 1, 2), 2)):
        b = _solver(ebos, name)
        np.random.seed(c["init_seed"])
        flows = b.estimate_batch([wins[i][1] for i in order], frames=[wins[i][0] for i in order], max_batch=max_batch)
        assert flows.shape == (3, 2) + tuple(c["shape"])
        for j, i in enumerate(order):   # (max_batch = 2: two launch sets, one table)
            assert np.array_equal(flows[j], singles[i]), (order, j)
            assert np.array_equal(b.estimate_indices_batch[j], indices[i]) and np.array_equal(b.best_values_batch[j], values[i])
        assert len(b.best_values_batch) == 3 and np.array_equal(b.best_values, values[order[-1]]) and b.iter_cnt == 3
    assert one.iter_cnt == 3


def test_evaluator_equals_the_loop_over_estimate(ebos, tmp_path):
    """configs/eklt_patch_sweep.yaml on the synthetic recording: ``RecordingEvaluator.run(max_batch=2)`` (the windows' polarity
    images built on the device from the raw columns, two windows per launch) equals the driver's loop over ``estimate``."""
    import yaml

    from event_based_bos_amd import evaluation as EV
    from event_based_bos_amd.utils import propagate_config
    from test_gpu_evaluation import _driver_loop, _recording, _same_dicts, _Viz

    with open(os.path.join(ROOT, "configs", "eklt_patch_sweep.yaml")) as f:
        cfg = yaml.safe_load(f)
    shape = (cfg["data"]["height"], cfg["data"]["width"])
    events, frames, stamps = _recording(ebos, tmp_path / "rec", shape, 6, 6000)
    cfg["evaluation"]["time_list"] = [[float(stamps[0]) + 0.004, float(stamps[-1]) + 0.004]]
    cfg = propagate_config(cfg)
    d = cfg["data"]

    def make(save_dir):
        return ebos.solver.collections["generative_patch_independent"]((d["height"], d["width"]), (d["crop_height"], d["crop_width"]), {},
                                                                       copy.deepcopy(cfg["solver"]), _Viz(save_dir))

    want = _driver_loop(ebos, cfg, events, frames, make(tmp_path / "loop"))
    assert len(want["e0"]) >= 3
    solv = make(tmp_path / "eval")
    res = EV.RecordingEvaluator(cfg, events, frames, solv).run(max_batch=2, keep_flows=True)
    _same_dicts(res.errors_without_mask, want["e0"])
    _same_dicts(res.errors_with_mask, want["e1"])
    assert res.timestamps == want["ts"]
    assert all(np.isfinite(e["EPE"]) for e in res.errors_with_mask)
    assert 0 < len(solv.estimate_indices) < solv.n_patch   # the thresholding dropped some patches, not all
