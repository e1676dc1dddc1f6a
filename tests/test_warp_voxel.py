"""CPU checks of the time-aware warp (``motion_model="dense-flow-voxel"``): tests/_warp_voxel_ref.py, the restatement the GPU tests
compare with, is pinned to the reference's own warp and splat by composition (tests/golden/golden_warp_voxel.npz, written by
make_golden_warp_voxel.py) with ``array_equal``; the bin rule is checked on its edge cases by hand; the product's argument errors and
its no-GPU behaviour need no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _warp_voxel_ref as R  # noqa: E402

from oracle import ebos_oracle as O  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "golden_warp_voxel.npz"))
DIRECTIONS = ("first", "middle", "last", 0.3, "before", "after")     # as in make_golden_warp_voxel.py
BINS = (1, 2, 3, 5)
CONV = {"np": lambda a: torch.from_numpy(a.copy()), "t64": lambda a: torch.from_numpy(a.copy()),
        "t32": lambda a: torch.from_numpy(a.astype(np.float32))}
WARP_KEYS = sorted(k for k in G.files if k.startswith("warp_"))


def test_the_fixture_holds_the_cases_the_tests_count_on():
    assert len(WARP_KEYS) == 4 * 6 * 3 + 4 * 3 * 2 + 2 * 2 * 2 * 2
    assert {k.split("_")[1] for k in WARP_KEYS} == {"unit", "sec"} and {k.split("_")[2] for k in WARP_KEYS} == {"1", "2"}
    for w, lo, hi in (("unit", 0.0, 1.0), ("sec", 0.25, 3.75)):
        for b in (1, 2):
            t = G[f"ev_{w}_{b}"][..., 2]
            assert (t.min(axis=-1) == lo).all() and (t.max(axis=-1) == hi).all()


@pytest.mark.parametrize("key", WARP_KEYS)
def test_restatement_equals_the_reference_composed_bin_by_bin(key):
    _, w, b, T, d, tag = key.split("_")
    ev, vx = CONV[tag](G[f"ev_{w}_{b}"]), CONV[tag](G[f"vox_{T}_{b}"])
    want = G[key]
    assert want.dtype == (np.float32 if tag == "t32" else np.float64)
    for batched in ((True,) if b == "2" else (True, False)):
        e, v = (ev, vx) if batched else (ev[0], vx[0])
        got = R.warp_voxel(e, v, DIRECTIONS[int(d)], normalize_t=False).numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want), key
        if w == "unit":   # times span exactly [0, 1]: the period is exactly 1, dividing by it changes nothing
            got = R.warp_voxel(e, v, DIRECTIONS[int(d)], normalize_t=True).numpy()
            assert np.array_equal(got, want), key + " normalize_t"


@pytest.mark.parametrize("T", BINS)
@pytest.mark.parametrize("pad", [0, 2])
def test_restated_iwe_equals_the_references_splat_of_the_composed_warp(T, pad):
    ev, vx = torch.from_numpy(G["ev_unit_1"][0]), torch.from_numpy(G[f"vox_{T}_1"][0])
    assert np.array_equal(R.iwe_voxel(ev, vx, "middle", True, (pad, pad)).numpy(), G[f"iwe_{T}_{pad}"])
    w = torch.from_numpy(G["iwe_weight"])
    assert np.array_equal(R.iwe_voxel(ev, vx, "middle", True, (pad, pad), w).numpy(), G[f"iwe_{T}_{pad}_w"])


def test_bin_rule_on_its_edges():
    t = np.array([2.0, 6.0, 4.0, 3.0, 5.0, 2.5, 5.999])           # tmin = 2, tmax = 6: tau = 0, 1, 1/2, 1/4, 3/4, 1/8, ~1
    assert R.time_bins(t, 1).tolist() == [0] * 7                 # T == 1: every event in bin 0
    assert R.time_bins(t, 2).tolist() == [0, 1, 1, 0, 1, 0, 1]   # t == tmin -> 0; t == tmax -> T - 1; tau = 1/2 opens bin 1
    assert R.time_bins(t, 4).tolist() == [0, 3, 2, 1, 3, 0, 3]   # tau = 1/4, 1/2, 3/4 open bins 1, 2, 3
    assert R.time_bins(np.full(5, 7.25), 4).tolist() == [0] * 5  # all times equal
    assert R.time_bins(np.array([[0.0, 1.0, 0.5], [10.0, 30.0, 20.0]]), 2).tolist() == [[0, 1, 1], [0, 1, 1]]   # per batch row
    # float32 times are widened exactly: the bin of a float32 time is the bin of the same value as a float64
    t32 = np.random.RandomState(3).uniform(0, 1, 1000).astype(np.float32)
    assert np.array_equal(R.time_bins(t32, 5), R.time_bins(t32.astype(np.float64), 5))
    assert R.time_bins(t, 3).dtype == np.int64


def test_the_bin_does_not_depend_on_the_direction_and_only_moves_the_gather():
    ev, vx = torch.from_numpy(G["ev_sec_1"][0]), torch.from_numpy(G["vox_3_1"][0])
    k = R.time_bins(ev[:, 2], 3)
    for direction in DIRECTIONS:
        got = R.warp_voxel(ev, vx, direction)[0]
        for b in range(3):
            want = O.warp_dense_torch(ev, vx[b], direction, False)
            assert torch.equal(got[k == b], want[k == b])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("normalize_t", [False, True])
def test_one_bin_restates_plain_dense_flow(dtype, normalize_t):
    ev, flow = torch.from_numpy(G["ev_sec_2"]).to(dtype), torch.from_numpy(G["vox_2_2"][:, :1]).to(dtype)
    for direction in DIRECTIONS:
        want = O.warp_dense_torch(ev, flow[:, 0], direction, normalize_t)
        assert torch.equal(R.warp_voxel(ev, flow, direction, normalize_t), want.reshape(2, -1, 4))


# ---------------------------------------------------------------------------------------------- the product, without a GPU
def _ev(n=6):
    ev = np.zeros((n, 4))
    ev[:, 2] = np.linspace(0, 1, n)
    return ev


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_for_the_voxel_model():
    import event_based_bos_amd as ebos

    w = ebos.Warp((4, 5))
    with pytest.raises(ebos.HipUnavailableError):
        w.warp_event(_ev(), np.zeros((3, 2, 4, 5)), "dense-flow-voxel")
    with pytest.raises(ebos.HipUnavailableError):
        w.warp_event(torch.from_numpy(_ev()), torch.zeros((3, 2, 4, 5), dtype=torch.float64), "dense-flow-voxel", "middle")
    with pytest.raises(ebos.HipUnavailableError):
        w.warp_event_from_optical_flow_voxel(_ev(), np.zeros((3, 2, 4, 5)), 0.5)
    with pytest.raises(ebos.HipUnavailableError):
        ebos.ops.time_bins(torch.zeros(1, 5, 4), 3)


def test_argument_errors_come_before_the_gpu_is_asked_for():
    import event_based_bos_amd as ebos

    w = ebos.Warp((4, 5))
    for bad in (np.zeros((2, 4, 5)), np.zeros((1, 3, 2, 4, 5)), np.zeros((3, 3, 4, 5)), np.zeros((0, 2, 4, 5)), np.zeros((256, 2, 4, 5))):
        with pytest.raises(ValueError):
            w.warp_event(_ev(), bad, "dense-flow-voxel")
        with pytest.raises(ValueError):
            w.warp_event_from_optical_flow_voxel(_ev(), bad, 0.0)
    with pytest.raises(ValueError):   # batched events take a batched voxel
        w.warp_event(np.zeros((2, 6, 4)), np.zeros((3, 2, 4, 5)), "dense-flow-voxel")
    with pytest.raises(ValueError):   # the direction is checked first, as for every model
        w.warp_event(_ev(), np.zeros((3, 2, 4, 5)), "dense-flow-voxel", direction=1)
    for T in (0, 256, -1):
        with pytest.raises(ValueError):
            ebos.ops.time_bins(torch.zeros(1, 5, 4), T)
    with pytest.raises(ValueError):
        ebos.ops.warp_voxel(torch.zeros(1, 5, 4), torch.zeros(1, 3, 3, 4, 5), 0, 0.0, False)


def test_other_models_and_the_helpers_are_as_they_were():
    import event_based_bos_amd as ebos

    w = ebos.Warp((4, 5))
    with pytest.raises(ebos.MotionModelKeyError):
        w.warp_event(_ev(), np.zeros((2, 4, 5)), "affine")
    with pytest.raises(ebos.MotionModelKeyError):
        w.warp_event(_ev(), np.zeros((3, 2, 4, 5)), "dense-flow-voxel-optimized")
    for helper in (w.get_key_names, w.get_motion_vector_size):
        with pytest.raises(ebos.MotionModelKeyError):
            helper("dense-flow-voxel")
    with pytest.raises(ebos.MotionModelKeyError):
        w.motion_model_to_motion("dense-flow-voxel", {})
    with pytest.raises(ebos.MotionModelKeyError):
        w.motion_model_from_motion(np.zeros(2), "dense-flow-voxel")


def test_a_time_aware_plan_needs_the_full_build():
    import event_based_bos_amd as ebos

    ev = torch.zeros(5, 4)
    for kwargs in ({"emit": "compact"}, {"deferred": True}, {"emit": "compact", "tile": None}):
        with pytest.raises(NotImplementedError, match='emit="full"'):
            ebos.EventPlan.build(ev, (4, 5), time_bin=3, **kwargs)
    with pytest.raises(NotImplementedError, match='emit="full"'):
        ebos.EventPlan.build_raw(torch.zeros(5, dtype=torch.int16), torch.zeros(5, dtype=torch.int16), torch.zeros(5, dtype=torch.int64),
                                 torch.zeros(5, dtype=torch.uint8), (4, 5), time_bin=3)
    for T in (0, 256):
        with pytest.raises(ValueError):
            ebos.EventPlan.build(ev, (4, 5), time_bin=T)


def test_the_solver_block_is_validated_without_a_gpu():
    from event_based_bos_amd.solver.contrast_maximization import parse_time_aware

    assert parse_time_aware(None) is None
    assert parse_time_aware({"time_bin": 5}) == {"time_bin": 5, "scheme": "upwind", "t0_location": "middle", "clamp": None}
    assert parse_time_aware({"time_bin": 3, "scheme": "burgers", "t0_location": "first", "clamp": 2})["clamp"] == 2.0
    for bad in ({}, {"time_bin": 0}, {"time_bin": 256}, {"time_bin": 3, "scheme": "bilinear"}, {"time_bin": 3, "t0_location": "last"},
                {"time_bin": 3, "bins": 2}):
        with pytest.raises(ValueError):
            parse_time_aware(bad)
