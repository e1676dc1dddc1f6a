"""GPU checks of the flow-error metrics (event_based_bos_amd/flow_error.py, csrc/flow_error.hip): every case of
tests/golden/golden_flow_error.npz through the reference-named functions, the batched entry against single calls, determinism,
strided ROI views, a 64-window batch, the validation errors and the solver's end-to-end evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

from _flow_error_cases import CASES, KEYS, ROI, case_inputs, restated_flow_error, solver_events

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_flow_error.npz")
DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _fe():
    from event_based_bos_amd import flow_error
    return flow_error


def assert_close(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rel, atol=0)


def _exact_counts(table, want_table):
    """float64: the mask counts and the threshold counts (ratio * n) are exact."""
    np.testing.assert_array_equal(table[:, 8], want_table[:, 8])
    n = want_table[:, 8:9] + 1e-5
    np.testing.assert_array_equal(np.rint(table[:, 1:7] * n), np.rint(want_table[:, 1:7] * n))
    np.testing.assert_array_equal(table[:, 1:7], want_table[:, 1:7])


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases(golden, name):
    fe = _fe()
    gt, pred, mask, ts = case_inputs(name, golden)
    want = golden[name + "_ref"]
    if CASES[name] == "tensor32":
        got = fe.calculate_flow_error_tensor(torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV),
                                             torch.from_numpy(mask).to(DEV), torch.from_numpy(ts).to(DEV))
        assert all(v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda for v in got.values())
        assert_close([got[k].item() for k in KEYS], want, 1e-5)
        return
    got = fe.calculate_flow_error_numpy(gt, pred, event_mask=mask)
    assert list(got) == list(KEYS) and all(type(v) is np.float64 for v in got.values())
    assert_close([got[k] for k in KEYS], want, 1e-12)
    # exact counts against the restatement (its e is the reference's, bit for bit)
    table, _ = fe.flow_error_batch(gt, pred, mask)
    want_table, _ = restated_flow_error(gt, pred, mask)
    _exact_counts(table.cpu().numpy(), want_table)
    # the tensor variant on device float64 tensors gives the same values
    gt_t = torch.from_numpy(np.ascontiguousarray(gt)).to(DEV)
    pred_t = torch.from_numpy(np.ascontiguousarray(pred)).to(DEV)
    m_t = None if mask is None else torch.from_numpy(mask).to(DEV)
    tens = fe.calculate_flow_error_tensor(gt_t, pred_t, m_t)
    assert all(v.dtype == torch.float64 and v.is_cuda for v in tens.values())
    np.testing.assert_array_equal([tens[k].item() for k in KEYS], [got[k] for k in KEYS])


def test_batch_items_equal_single_calls_and_runs_are_bit_identical():
    fe = _fe()
    gt, pred, mask, _ = case_inputs("batch3")
    for dtype in (torch.float64, torch.float32):
        g, p = torch.from_numpy(gt).to(DEV, dtype), torch.from_numpy(pred).to(DEV, dtype)
        m = torch.from_numpy(mask).to(DEV)
        ts = torch.tensor([0.5, 1.0, 3.0], dtype=dtype, device=DEV)
        table, means = fe.flow_error_batch(g, p, m, ts)
        for b in range(3):
            one, _ = fe.flow_error_batch(g[b:b + 1], p[b:b + 1], m[b:b + 1], ts[b:b + 1])
            assert torch.equal(one[0], table[b]), (dtype, b)
        again = fe.flow_error_batch(g, p, m, ts)
        assert torch.equal(again[0], table) and torch.equal(again[1], means)
        np.testing.assert_allclose(means.cpu().numpy(), table.cpu().numpy().mean(axis=0), rtol=1e-14)


def test_strided_roi_views_equal_contiguous_copies():
    fe = _fe()
    rs = np.random.RandomState(21)
    for dtype in (torch.float64, torch.float32):
        full_gt = torch.from_numpy(rs.uniform(-8, 8, (2, 2, 720, 1280))).to(DEV, dtype)
        full_pr = full_gt + torch.from_numpy(rs.normal(0, 3, (2, 2, 720, 1280))).to(DEV, dtype)
        mask_full = torch.from_numpy(rs.uniform(size=(2, 1, 720, 1280)) < 0.4).to(DEV)
        for cols in ((320, 960), (321, 960)):                   # vector loads, and the scalar path of an unaligned view
            sl = (slice(None), slice(None), slice(0, 720), slice(*cols))
            view_g, view_p, view_m = full_gt[sl], full_pr[sl], mask_full[sl]
            assert not view_g.is_contiguous()
            a = fe.flow_error_batch(view_g, view_p, view_m)[0]
            b = fe.flow_error_batch(view_g.contiguous(), view_p.contiguous(), view_m.contiguous())[0]
            assert torch.equal(a, b), (dtype, cols)
        # a channel-last layout is made contiguous on the host side
        cl = full_gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert torch.equal(fe.flow_error_batch(cl, full_pr)[0], fe.flow_error_batch(full_gt, full_pr)[0])


def test_64_windows_in_one_call():
    fe = _fe()
    rs = np.random.RandomState(22)
    gt = rs.uniform(-6, 6, (64, 2, 260, 346))
    pred = gt + rs.normal(0, 2, gt.shape)
    mask = rs.uniform(size=(64, 1, 260, 346)) < 0.3
    table, means = fe.flow_error_batch(torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV), torch.from_numpy(mask).to(DEV))
    want, want_means = restated_flow_error(gt, pred, mask)
    got = table.cpu().numpy()
    _exact_counts(got, want)
    np.testing.assert_allclose(got[:, [0, 7]], want[:, [0, 7]], rtol=1e-12)
    np.testing.assert_allclose(means.cpu().numpy(), want_means, rtol=1e-12)


def test_clamped_angle_is_finite_for_a_perfect_prediction():
    fe = _fe()
    gt, pred, _, _ = case_inputs("pred_eq_gt")
    _, plain = fe.flow_error_batch(gt, pred)
    _, clamped = fe.flow_error_batch(gt, pred, clamp_angle=True)
    # (cosines that round just below 1 still give acos of a few 1e-8)
    assert np.isnan(plain[7].item()) and 0.0 <= clamped[7].item() < 1e-7
    assert torch.equal(plain[:7], clamped[:7])


def test_validation_errors():
    fe = _fe()
    f = torch.zeros((2, 2, 8, 9), device=DEV)
    with pytest.raises(ValueError):
        fe.flow_error_batch(f[0], f[0])                                              # rank
    with pytest.raises(ValueError):
        fe.flow_error_batch(f, torch.zeros((2, 2, 8, 10), device=DEV))              # shape mismatch
    with pytest.raises(ValueError):
        fe.flow_error_batch(f, f, torch.ones((3, 1, 8, 9), dtype=torch.bool, device=DEV))   # mask does not broadcast
    with pytest.raises(ValueError):
        fe.flow_error_batch(f, f, torch.ones((2, 2, 8, 9), dtype=torch.bool, device=DEV))   # two-channel mask
    with pytest.raises(ValueError):
        fe.flow_error_batch(f.to(torch.int32), f.to(torch.int32))                      # not floating
    with pytest.raises(ValueError):
        fe.flow_error_batch(f, f, time_scale=torch.ones(3, device=DEV))              # one time scale per item


def test_solver_end_to_end():
    """ContrastMaximization.estimate on run_cmax's synthetic window, then the driver's two evaluations, against the restatement."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_cmax
    import event_based_bos_amd as ebos

    cfg = run_cmax.load_config(os.path.join(ROOT, "tests", "golden", "config_hot_plate1.json"))
    d, cp = cfg["data"], cfg.setdefault("common_params", {})
    d["height"], d["width"], d["n_events"] = 260, 346, 100_000
    cp.update(xmin=0, xmax=260, ymin=40, ymax=300)
    ebos.utils.propagate_config(cfg)
    scfg = cfg["solver"]
    scfg["method"], scfg["cost_with_weight"] = "contrast_maximization", {"image_variance": 1.0}
    scfg.setdefault("optimizer", {})["n_iter"] = 50
    events, shape = run_cmax.synthetic_window(cfg)
    solver = ebos.solver.collections["contrast_maximization"](shape, (d["crop_height"], d["crop_width"]), calibration_parameter=None,
                                                              solver_config=scfg, visualize_module=None)
    events, _ = solver.preprocess(events)
    flow = solver.estimate(events)
    truth = run_cmax.dense_truth(d)
    r = (slice(None), slice(cp["xmin"], cp["xmax"]), slice(cp["ymin"], cp["ymax"]))
    roi = {k: cp[k] for k in ("xmin", "xmax", "ymin", "ymax")}
    without = solver.calculate_flow_error(flow[r], truth[r])
    with_mask = solver.calculate_flow_error(flow[r], truth[r], events=events, roi=roi)
    mask = solver.orig_imager.create_eventmask(torch.from_numpy(events).to(DEV))[:, r[1], r[2]].cpu().numpy()
    assert 0 < mask.mean() < 1
    for got, m in ((without, None), (with_mask, mask)):
        _, want = restated_flow_error(truth[r][None], flow[r][None], m)
        assert_close([got[k] for k in KEYS], want[:8], 1e-12)
    assert without["EPE"] > 0 and with_mask["EPE"] != without["EPE"]


def test_solver_case_mask_from_events(golden):
    """The solver fixture case through SolverBase: the mask comes from create_eventmask of the events on the device."""
    import event_based_bos_amd as ebos

    gt, pred, _, _ = case_inputs("solver_roi", golden)
    solver = ebos.solver.SolverBase((720, 1280), (720, 640), solver_config={})
    got = solver.calculate_flow_error(pred[0], gt[0], events=solver_events(), roi=ROI)
    assert_close([got[k] for k in KEYS], golden["solver_roi_ref"], 1e-12)
