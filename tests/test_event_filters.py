"""CPU checks of the event filters (event_based_bos_amd/event_filters.py, csrc/event_filters.hip): the config plumbing of
EventFilter and SolverBase, the C ABI entries, and the numpy restatement of the reference loops the GPU tests check large
windows against, pinned on the reference's own outputs (tests/golden/golden_filters.npz)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _filter_ref import baf_numpy, hot_numpy, load_golden_filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_filters.npz")
HW = (260, 346)


@pytest.fixture(scope="module")
def golden():
    return load_golden_filters(GOLDEN)


def _cases(g, prefix):
    return sorted({k[:-len("_params")] for k in g if k.startswith(prefix) and k.endswith("_params")})


def test_restatement_matches_the_reference_baf(golden):
    cases = _cases(golden, "baf_")
    assert len(cases) >= 10
    for c in cases:
        dt, k, s = golden[c + "_params"]
        kept, m = baf_numpy(golden[c + "_events"], HW, dt, int(k), int(s), golden[c + "_m0"])
        np.testing.assert_array_equal(kept, golden[c + "_kept"], err_msg=c)
        np.testing.assert_array_equal(m, golden[c + "_map"], err_msg=c)


def test_restatement_matches_the_reference_hot(golden):
    for c in ("hot_int", "hot_int_f32"):
        np.testing.assert_array_equal(hot_numpy(golden[c + "_events"], HW, golden[c + "_params"][0]), golden[c + "_kept"])


def test_fixture_covers_the_issue_cases(golden):
    ev = golden["baf_k1s1_events"]
    drop = 1 - len(golden["baf_k1s1_kept"]) / len(ev)
    assert 0.2 <= drop <= 0.8
    assert (np.diff(ev[:, 2]) < 0).any()                                   # times out of order
    b = golden["baf_border_events"]
    assert ((b[:, 0] == 0) & (b[:, 1] == 0)).any() and ((b[:, 0] == HW[0] - 1) & (b[:, 1] == HW[1] - 1)).any()
    assert (golden["baf_frac_events"][:, :2] % 1 != 0).any()
    assert golden["baf_m0_m0"].any()
    # pixels whose count equals the threshold are kept, one above it dropped
    ev, kept, th = golden["hot_int_events"], golden["hot_int_kept"], golden["hot_int_params"][0]
    key = ev[:, 0].astype(np.int64) * HW[1] + ev[:, 1].astype(np.int64)
    cnt = np.bincount(key, minlength=HW[0] * HW[1])
    kk = kept[:, 0].astype(np.int64) * HW[1] + kept[:, 1].astype(np.int64)
    assert (cnt[kk] == th).any() and (cnt == th + 1).any() and not (cnt[kk] > th).any()
    assert len(golden["seq_1_w2_out"]) < 10                                # the 10-event rule


def test_the_module_exists_and_is_reexported():
    from event_based_bos_amd import event_filters, utils

    for name in ("background_activity_filter", "continuous_background_activity_filter", "hot_pixel_filter", "EventFilter"):
        assert getattr(utils, name) is getattr(event_filters, name)


def test_event_filter_config_plumbing():
    from event_based_bos_amd.event_filters import EventFilter

    p = {"BAF_dt": 0.005, "BAF_ksize": 1, "BAF_num_support_event": 1, "BAF_continuous_update": True, "HOT_thresh": 10}
    f = EventFilter(HW, {"filters": ["HOT", "BAF"], "parameters": p})
    assert f.filters == ["HOT", "BAF"] and f.continuous_update and f.time_map is None
    f = EventFilter(HW, {"filters": ["BAF", "HOT"], "parameters": dict(p, xmin=0, xmax=10, ymin=0, ymax=10)})
    assert f.filters == ["CROP", "BAF", "HOT"]
    assert [fn.__name__ for fn in f.filter_func] == ["crop", "background_activity_filter", "hot_pixel_filter"]
    with pytest.raises(KeyError):
        EventFilter(HW, {"filters": ["BAF", "FLICKER"], "parameters": p})
    assert EventFilter(HW, {"filters": None, "parameters": dict(xmin=0, xmax=1, ymin=0, ymax=1)}).filters == ["CROP"]
    assert EventFilter(HW, {"parameters": {}}).filters == []
    assert not EventFilter(HW, {"filters": ["BAF"], "parameters": dict(p, BAF_continuous_update=False)}).continuous_update


def _solver(filter_section):
    import event_based_bos_amd as ebos

    cfg = {"method": "contrast_maximization", "motion_model": "dense-flow", "warp_direction": "first",
           "cost_with_weight": {"image_variance": 1.0}, "optimizer": {"method": "Adam", "n_iter": 2, "parameters": {"lr": 0.1}}}
    if filter_section is not None:
        cfg["filter"] = filter_section
    return ebos.solver.collections["contrast_maximization"](HW, HW, solver_config=cfg)


def test_solver_builds_the_filter_only_when_filters_are_listed():
    roi = {"xmin": 0, "xmax": 100, "ymin": 0, "ymax": 200}
    for section in (None, {"parameters": roi}, {"filters": None, "parameters": roi}, {"filters": [], "parameters": roi}):
        s = _solver(section)
        assert s.filter_set is None          # CROP alone: preprocess takes exactly the old path
    s = _solver({"filters": ["BAF", "HOT"], "parameters": dict(roi, BAF_dt=0.005, BAF_ksize=1, BAF_num_support_event=1, HOT_thresh=10)})
    assert s.filter_set is not None and s.filter_set.filters == ["CROP", "BAF", "HOT"] and s.roi == (0, 100, 0, 200)
    with pytest.raises(KeyError):
        _solver({"filters": ["NOPE"], "parameters": roi})


HEADER = os.path.join(ROOT, "include", "ebos_hip.h")
NEW = ("ebos_event_filter_scratch_bytes", "ebos_baf_mask", "ebos_hot_mask", "ebos_filter_compact")


def test_header_entries_and_ctypes_table():
    from event_based_bos_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_hip.SIGNATURES[name][1]), name
    assert "#define EBOS_ABI_VERSION 2" in text and _hip.ABI_VERSION == 2
    doc = open(HEADER).read()
    assert "src/utils/event_filters.py" in doc and ":46-97" in doc and ":100-128" in doc


def test_event_source_struct_layout_matches_the_ctypes_mirror(tmp_path):
    from event_based_bos_amd import _hip

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in _hip.EventSource._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ebos_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(ebos_event_source));']
    lines += [f'  printf("%zu\\n", offsetof(ebos_event_source, {f}));' for f in fields]
    lines += ['  return EBOS_FILTER_SRC_RAW64 == 3 && EBOS_FILTER_STATUS_CLIPPED == 1 ? 0 : 1;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0
    want = [C.sizeof(_hip.EventSource)] + [getattr(_hip.EventSource, f).offset for f in fields]
    assert [int(v) for v in run.stdout.split()] == want
    assert (_hip.FILTER_SRC_F32, _hip.FILTER_SRC_F64, _hip.FILTER_SRC_RAW32, _hip.FILTER_SRC_RAW64) == (0, 1, 2, 3)


def test_host_side_validation_without_a_gpu():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    lib = _hip.load_library()
    b = lib.ebos_event_filter_scratch_bytes(100_000, 260, 346)
    assert b >= 100_000 * 32 and lib.ebos_event_filter_scratch_bytes(2_000_000, 720, 1280) >= b
    assert lib.ebos_event_filter_scratch_bytes(-1, 260, 346) == 0 and lib.ebos_event_filter_scratch_bytes(10, 0, 346) == 0
    src = _hip.EventSource(kind=_hip.FILTER_SRC_F64, layout=0x24, n=0)
    # out-of-range ksize / num_support_event: EBOS_ERR_UNSUPPORTED with a message, before any HIP call
    dummy = C.c_void_p(16)
    rc = lib.ebos_baf_mask(C.byref(src), 260, 346, None, None, 0.005, 8, 1, None, dummy, dummy, dummy, dummy, dummy, b, None)
    assert rc == -3 and b"ksize" in lib.ebos_last_error()
    rc = lib.ebos_baf_mask(C.byref(src), 260, 346, None, None, 0.005, 1, 16, None, dummy, dummy, dummy, dummy, dummy, b, None)
    assert rc == -3
    bad = _hip.EventSource(kind=7, layout=0x24, n=0)
    assert lib.ebos_hot_mask(C.byref(bad), 260, 346, None, None, 10.0, None, dummy, dummy, dummy, dummy, b, None) == -1
