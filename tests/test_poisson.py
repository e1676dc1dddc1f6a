"""CPU checks of the Poisson integration (event_based_bos_amd/poisson.py, csrc/poisson.hip): the dense-DST restatement the GPU tests
hold the kernel against, pinned on the reference's own outputs (tests/golden/golden_poisson.npz); the C ABI entries; the names
``utils`` re-exports; validation that needs no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from _poisson_cases import CASES, case_inputs, golden_case, stored_rows
from _poisson_ref import dst_matrix, restated_image, restated_poisson

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_poisson.npz")
HEADER = os.path.join(ROOT, "include", "ebos_hip.h")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference(golden, name):
    flow, boundary = case_inputs(name)
    rows, want, u8, absmax = golden_case(golden, name)
    got = restated_poisson(flow[1], flow[0], boundary)
    assert got.dtype == want.dtype == boundary.dtype
    assert abs(float(np.abs(got).max()) - absmax) <= 1e-12 * absmax
    err = np.abs(got[rows].astype(np.float64) - want).max() / absmax
    assert err <= 1e-12, err
    np.testing.assert_array_equal(restated_image(got), u8)   # (the whole picture, also where the field is not stored)


def test_fixture_covers_the_issue_cases(golden):
    shapes = {CASES[n][:2] for n in CASES}
    assert {(3, 3), (4, 5), (31, 47), (64, 64), (260, 346)} <= shapes
    assert {CASES[n][4] for n in CASES} == {"zero", "rand"}
    assert {CASES[n][2] for n in CASES} == {np.float32, np.float64}
    assert os.path.getsize(GOLDEN) < 512 * 1024
    for n in CASES:
        flow, boundary = case_inputs(n)
        rows, P, u8, absmax = golden_case(golden, n)
        H, W = boundary.shape
        r = np.arange(H)[rows]
        assert P.shape == (len(r), W) and u8.shape == (H, W) and r[0] == 0 and r[-1] == H - 1
        np.testing.assert_array_equal(P[0], boundary[0])                 # the frame is the boundary's
        np.testing.assert_array_equal(P[-1], boundary[-1])
        np.testing.assert_array_equal(P[:, -1], boundary[r, -1])
        assert np.abs(P[1:-1, 1:-1]).max() > 0 and np.abs(P).max() <= absmax
    assert stored_rows("s260x346_f64_zero") is not None and stored_rows("s64x64_f64_rand") is None


def test_dst_matrix_is_orthonormal():
    for N in (1, 2, 7, 64, 359):
        S = dst_matrix(N)
        np.testing.assert_allclose(S @ S.T, np.eye(N), atol=1e-13)


def test_the_module_exists_and_is_reexported():
    import event_based_bos_amd as ebos

    for name in ("poisson_reconstruct", "poisson_reconstruct_batch", "poisson_image", "standardize_image_center"):
        assert getattr(ebos.utils, name) is getattr(ebos.poisson, name)
    assert list(inspect.signature(ebos.utils.poisson_reconstruct).parameters) == ["grady", "gradx", "boundarysrc"]
    sig = inspect.signature(ebos.utils.standardize_image_center).parameters
    assert list(sig) == ["array", "old_center", "new_center", "new_max"]
    assert (sig["old_center"].default, sig["new_center"].default, sig["new_max"].default) == (0, 128, 255)


def test_standardize_image_center_is_the_reference_formula():
    from event_based_bos_amd.utils import standardize_image_center

    a = np.array([[-2.0, 1.0], [0.5, 0.0]], dtype=np.float32)
    got = standardize_image_center(a)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, (a - 0) / np.float32(2.0) * 127 + 128)


def test_header_entries_and_ctypes_table():
    from event_based_bos_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("ebos_poisson_scratch_bytes", "ebos_poisson_reconstruct"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_hip.SIGNATURES[name][1]), name
    assert re.search(r"EBOS_POISSON_F32 = 0", text) and re.search(r"EBOS_POISSON_F64 = 1", text)
    assert (_hip.POISSON_F32, _hip.POISSON_F64) == (0, 1)
    assert "#define EBOS_ABI_VERSION 2" in text and _hip.ABI_VERSION == 2
    from event_based_bos_amd.build import SOURCES
    assert "poisson.hip" in SOURCES


def test_validation_without_a_gpu():
    from event_based_bos_amd import poisson

    f = np.zeros((2, 4, 5))
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct_batch(np.zeros((2, 2, 5)))                    # H < 3
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct_batch(np.zeros((1, 2, 4, 2)))                 # W < 3
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct_batch(np.zeros((1, 3, 4, 5)))                 # components
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct_batch(f.astype(np.int32))                     # dtype
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct_batch(f, np.zeros((4, 6)))                    # boundary shape
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct_batch(f, np.zeros((4, 5), dtype=np.float16))  # boundary dtype
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct(f[1], f[0], np.zeros((4, 6)))                 # shapes differ
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct(f[1][None], f[0][None], np.zeros((1, 4, 5)))  # rank
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct(f[1, :2], f[0, :2], np.zeros((2, 5)))         # H < 3
    with pytest.raises(ValueError):
        poisson.poisson_reconstruct(f[1].astype(np.int64), f[0], np.zeros((4, 5)))
    with pytest.raises(ValueError):
        poisson.poisson_image(np.zeros((1, 2, 4, 5)), dtype=np.float32)           # not a torch dtype
