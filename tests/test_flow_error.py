"""CPU checks of the flow-error metrics (event_based_bos_amd/flow_error.py, csrc/flow_error.hip): the numpy restatement the GPU
tests hold the kernel against, pinned on the reference's own outputs (tests/golden/golden_flow_error.npz); the C ABI entries;
SolverBase's evaluation methods and the text file they write."""
import ast
import os
import re

import numpy as np
import pytest

from _flow_error_cases import CASES, KEYS, case_inputs, restated_flow_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_flow_error.npz")
HEADER = os.path.join(ROOT, "include", "ebos_hip.h")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def assert_matches_reference(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rel, atol=0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference(golden, name):
    gt, pred, mask, ts = case_inputs(name, golden)
    _, means = restated_flow_error(gt, pred, mask, ts)
    assert_matches_reference(means[:8], golden[name + "_ref"], 1e-5 if CASES[name] == "tensor32" else 1e-12)


def test_fixture_covers_the_issue_cases(golden):
    assert np.isnan(golden["pred_eq_gt_ref"][7])                        # AE of a perfect prediction
    assert np.isnan(golden["gt_special_ref"][0]) and np.isnan(golden["pred_nan_out_ref"][0])
    gt, pred, _, _ = case_inputs("thresholds")
    e = np.sqrt(((gt - pred) ** 2).sum(axis=1))
    for k in (1, 2, 3, 5, 10, 20):
        assert (e == k).sum() >= 3, k                                    # pixels exactly at every threshold
    gt, _, mask, _ = case_inputs("solver_roi", golden)
    assert gt.shape == (1, 2, 720, 640) and not gt.flags.c_contiguous and 0.05 < mask.mean() < 0.5
    table, _ = restated_flow_error(*case_inputs("batch3")[:3])
    assert len(set(table[:, 8])) == 3                                    # per-item masks


def test_the_module_exists_and_is_reexported():
    import event_based_bos_amd as ebos

    for name in ("calculate_flow_error_numpy", "calculate_flow_error_tensor", "flow_error_batch"):
        assert getattr(ebos.utils, name) is getattr(ebos.flow_error, name)
    assert ebos.flow_error.KEYS == KEYS


def test_header_entries_and_ctypes_table():
    from event_based_bos_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("ebos_flow_error_scratch_bytes", "ebos_flow_error"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_hip.SIGNATURES[name][1]), name
    assert re.search(r"EBOS_FLOW_ERROR_F32 = 0", text) and re.search(r"EBOS_FLOW_ERROR_F64 = 1", text)
    assert "#define EBOS_FLOW_ERROR_CLAMP_AE 1" in text and _hip.FLOW_ERROR_CLAMP_AE == 1
    assert (_hip.FLOW_ERROR_F32, _hip.FLOW_ERROR_F64) == (0, 1)
    assert "#define EBOS_ABI_VERSION 2" in text and _hip.ABI_VERSION == 2
    assert "src/utils/flow_utils.py:706-823" in open(HEADER).read()


def test_solver_base_has_the_evaluation_methods():
    import inspect

    from event_based_bos_amd.solver import ContrastMaximizationMixin, SolverBase

    assert list(inspect.signature(SolverBase.calculate_flow_error).parameters) == ["self", "pred_disp", "gt_flow", "timescale",
                                                                                   "events", "roi"]
    assert list(inspect.signature(SolverBase.save_flow_error_as_text).parameters) == ["self", "nth_frame", "flow_error_dict", "fname"]
    # the mixin does not carry them: composed over the reference's base, the reference's own methods stay in force
    assert "calculate_flow_error" not in vars(ContrastMaximizationMixin)
    assert "save_flow_error_as_text" not in vars(ContrastMaximizationMixin)


def _read_like_the_reference(path):
    """src/utils/misc.py:88-113's rule: "nan" -> "0.0", then ast.literal_eval of what follows "::"."""
    rows = []
    for line in open(path):
        line = line.replace("nan", "0.0")
        rows.append(ast.literal_eval(line[line.find("::") + 2: line.rfind("\n")]))
    return rows


def test_flow_error_text_parses_by_the_reference_rule(tmp_path):
    import torch

    from event_based_bos_amd.solver import SolverBase

    solv = SolverBase.__new__(SolverBase)          # no GPU: only the bookkeeping of the instance is used
    solv.visualizer = type("V", (), {"save_dir": str(tmp_path)})()
    solv.evaluation_text_list = []
    err = {"EPE": np.float64(1.25), "1PE": np.float64(np.nan), "AE": torch.tensor(0.5, dtype=torch.float64), "n": np.int64(3)}
    solv.save_flow_error_as_text(0, err, "flow_error_per_frame_with_mask.txt")
    solv.save_flow_error_as_text(1, {"EPE": 2.0, "1PE": 0.5, "AE": 0.25, "n": 4}, "flow_error_per_frame_with_mask.txt")
    solv.save_flow_error_as_text(1, {"t1": 0.1, "t2": 0.2}, "timestamps_per_frame.txt")
    path = os.path.join(str(tmp_path), "flow_error_per_frame_with_mask.txt")
    assert solv.evaluation_text_list == [path]
    rows = _read_like_the_reference(path)
    assert rows == [{"EPE": 1.25, "1PE": 0.0, "AE": 0.5, "n": 3}, {"EPE": 2.0, "1PE": 0.5, "AE": 0.25, "n": 4}]
    assert open(path).readline().startswith("frame 0::{")


def test_validation_without_a_gpu():
    from event_based_bos_amd import flow_error

    f = np.zeros((1, 2, 4, 5))
    with pytest.raises(ValueError):
        flow_error.calculate_flow_error_numpy(f[0], f[0])                    # rank
    with pytest.raises(ValueError):
        flow_error.calculate_flow_error_numpy(f, np.zeros((1, 2, 4, 6)))     # shape
    with pytest.raises(ValueError):
        flow_error.calculate_flow_error_numpy(f.astype(np.int32), f)          # dtype
    with pytest.raises(ValueError):
        flow_error.calculate_flow_error_numpy(np.zeros((1, 3, 4, 5)), np.zeros((1, 3, 4, 5)))  # channels
