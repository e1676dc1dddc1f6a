"""GPU checks of csrc/event_voxel.hip at the sizes where its kernels take another path than in tests/test_gpu_voxel.py: the
stride loops of the normaliser (beyond 65 536 voxels in the reduce, 262 144 in the map) and of the volume's range kernel (beyond
524 288 events), the ROI scans of the raw-column form beyond their first 256-event step, and one long window among short ones.
The inputs are tests/_voxel_size_cases.py; tests/test_voxel_size_cases.py pins their make-up on the CPU.

The votes are held to the bound of tests/test_gpu_voxel.py, per voxel |gpu - ref| <= 2 k u sum|w| and exactly 0 where nothing
votes.  The normaliser is held per voxel to |gpu - exact| <= 64 u max|v| / std against ``_voxel_ref.normalize_exact`` (moments by
``math.fsum``; the count of roundings behind the 64 is in ``_voxel_ref.normalize_bound``), zeros staying exactly zero.  A one-pass
sum / sum-of-squares variance misses that bar by more than two orders of magnitude on the +-1e6 grids, a stride loop that stops
after one trip by more than five (tests/test_voxel_size_cases.py shows both on a numpy model of the kernel's scheme).

Observed on an MI355X, worst share of the normaliser's bar per case (draw 0 / draw 1) -- the numpy model gives the same figures:
    (3, 151, 173)   drawn 0.0006 / 0.00004   plus1e6 0.0166 / 0.00003   minus1e6 0.0166 / 0.00003
    (5, 241, 319)   drawn 0.0003 / 0.0003    plus1e6 0.0001 / 0.0164    minus1e6 0.0001 / 0.0164
(maximum 0.0166: 6.8e-11 per voxel, a mean about one ulp of 1e6 from the exact one, divided by std = 1.73), and 0 on the GPU's own 384 395-voxel grid
of event votes.  Worst shares of the vote bound: 0.451 on the 524 588-event grid, 0.064 over the ten volumes, 0.166 over the raw
windows (the 300 000-event window 0.008).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _voxel_ref as R  # noqa: E402
import _voxel_size_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

within_bound = R.within_bound
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def normalize_alone(grid):
    """``grid`` (numpy) normalised as a batch of one -> a device tensor."""
    from event_based_bos_amd import _hip, event_voxel as V

    out = torch.from_numpy(grid).cuda().unsqueeze(0)
    V._normalize_(out, _hip.require_gpu())
    return out[0]


def alone(shape, variant, draw):
    return cached(("alone", shape, variant, draw), lambda: normalize_alone(S.norm_grid(shape, variant, draw)))


def within_normaliser_bar(got, grid, name):
    """Per voxel |got - normalize_exact(grid)| <= 64 u max|v| / std; the zeros of ``grid`` exactly zero, nothing else."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    exact, bound = R.normalize_exact(grid), R.normalize_bound(grid)
    assert got.shape == exact.shape and got.dtype == np.float64
    err = np.abs(got - exact)
    print(f"{name}: max |gpu - exact| {err.max():.3e}, bound {bound:.3e}, worst share of the bound {err.max() / bound:.4f}")
    assert (got[grid == 0] == 0).all()
    assert np.isfinite(got).all() and (err <= bound).all(), (float(err.max()), bound, int((err > bound).sum()))


# ---------------------------------------------------------------------------------------------------- 1. normaliser
@pytest.mark.parametrize("shape,variant,draw", S.norm_cases())
def test_normaliser_beyond_one_trip(shape, variant, draw):
    within_normaliser_bar(alone(shape, variant, draw), S.norm_grid(shape, variant, draw), f"{shape} {variant} draw {draw}")


@pytest.mark.parametrize("shape", S.NORM_SHAPES)
def test_normaliser_batch_has_the_bits_of_each_grid_alone(shape):
    from event_based_bos_amd import _hip, event_voxel as V

    cases = [(v, d) for d in S.NORM_DRAWS for v in S.NORM_VARIANTS]
    batch = torch.from_numpy(np.stack([S.norm_grid(shape, v, d) for v, d in cases])).cuda()
    assert batch.shape == (6,) + shape
    V._normalize_(batch, _hip.require_gpu())
    for b, (v, d) in enumerate(cases):
        assert torch.equal(batch[b], alone(shape, v, d)), (b, v, d)
    # a grid without a non-zero voxel and one with a single non-zero voxel (the last of the grid: only a lane's last trip reads
    # it) between two ordinary ones
    zero, one = np.zeros(shape), np.zeros(shape)
    one[-1, -1, -1] = 5.0
    grids = [S.norm_grid(shape, "plus1e6", 0), zero, one, S.norm_grid(shape, "drawn", 1)]
    batch = torch.from_numpy(np.stack(grids)).cuda()
    V._normalize_(batch, _hip.require_gpu())
    assert (batch[1] == 0).all()                              # stays as it is
    assert (batch[2] == 0).all()                              # std is NaN: centred only, 5 - 5
    assert torch.equal(batch[0], alone(shape, "plus1e6", 0)) and torch.equal(batch[3], alone(shape, "drawn", 1))


def same_as_normalised_own_grid(got, raw, name):
    """As tests/test_gpu_voxel.py judges ``normalize=True``: against the exact normaliser applied to the GPU's own un-normalised
    grid of another run (the votes of the two runs are added in different orders), equal non-zero masks, rel-L2 <= 1e-12."""
    got, want = got.cpu().numpy(), R.normalize_exact(raw.cpu().numpy())
    assert np.array_equal(got != 0, want != 0), name
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"{name}: rel-L2 {err:.3e}")
    assert err <= 1e-12, name


def test_voxel_grid_beyond_2048_workgroups_and_its_normalisation():
    from event_based_bos_amd import _hip, event_voxel as V

    x, y, pol, t = S.voxel_events()
    dev = tuple(torch.from_numpy(a).cuda() for a in (x, y, pol, t))
    raw = V.create_event_voxel(*dev, S.VOXEL_SHAPE)
    within_bound(raw, R.create_event_voxel(x, y, pol, t, S.VOXEL_SHAPE))
    own = raw.clone()
    V._normalize_(own.unsqueeze(0), _hip.require_gpu())
    within_normaliser_bar(own, raw.cpu().numpy(), "the normaliser on the GPU's own grid")
    same_as_normalised_own_grid(V.create_event_voxel(*dev, S.VOXEL_SHAPE, normalize=True), raw, "create_event_voxel(normalize=True)")


# ---------------------------------------------------------------------------------------------------- 2. discretised volume
@pytest.mark.parametrize("dtype,u", [(np.float64, 2.0 ** -53), (np.float32, 2.0 ** -24)])
@pytest.mark.parametrize("case", list(S.VOLUME_CASES))
def test_event_volume_beyond_one_trip(case, dtype, u):
    from event_based_bos_amd.utils import generate_discretized_event_volume

    ev = S.volume_events(case, dtype)
    got = generate_discretized_event_volume(torch.from_numpy(ev).cuda(), S.VOLUME_SIZE)
    assert got.is_cuda and got.dtype == torch.from_numpy(ev).dtype
    within_bound(got, R.generate_discretized_event_volume(ev, S.VOLUME_SIZE), u)


def test_nan_time_in_the_second_trip_raises():
    from event_based_bos_amd.utils import generate_discretized_event_volume

    ev = S.volume_events("both_tail")
    ev[S.NAN_INDEX, 2] = np.nan
    with pytest.raises(ValueError):
        generate_discretized_event_volume(torch.from_numpy(ev).cuda(), S.VOLUME_SIZE)


# ---------------------------------------------------------------------------------------------------- 3. windows of raw columns
def store_of(wide):
    def make():
        from event_based_bos_amd import RawEventStore

        cols, _ = S.raw_recording()
        return RawEventStore({**cols, "t": cols["t"].astype(np.int64) + (1 << 33)} if wide else cols)

    return cached(("store", wide), make)


def window_ref(store, window, roi):
    """(restatement of the window's grid or None for a window that is not valid, expected valid)"""
    def make():
        ev = S.kept_events(store, window, roi)
        if not S.expect_valid(ev):
            return None, 0
        H, W = (roi[1] - roi[0], roi[3] - roi[2]) if roi else S.SENSOR
        return R.voxel_of_events(ev, S.N_BINS, (H, W), origin=(roi[0], roi[2]) if roi else (0, 0)), 1

    return cached(("ref", id(store), window, roi), make)


def check_windows(store, ranges, roi):
    x0, x1, y0, y1 = roi or (0, S.SENSOR[0], 0, S.SENSOR[1])
    grids, valid = store.voxels(ranges, S.N_BINS, S.SENSOR, roi=None if roi is None else dict(xmin=x0, xmax=x1, ymin=y0, ymax=y1))
    assert grids.shape == (len(ranges), S.N_BINS, x1 - x0, y1 - y0) and grids.dtype == torch.float64 and grids.is_cuda
    refs = [window_ref(store, w, roi) for w in ranges]
    assert valid.tolist() == [ok for _, ok in refs]
    host = grids.cpu()
    for b, (ref, ok) in enumerate(refs):
        if ok:
            within_bound(host[b].numpy(), ref)
        else:
            assert (host[b] == 0).all(), b
    return grids, valid


@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
def test_windows_with_long_dropped_runs_and_one_long_window(wide):
    store = store_of(wide)
    win = S.raw_recording()[1]
    names = "abcdefg"
    ranges = [win[w] for w in names]
    grids, valid = check_windows(store, ranges, S.ROI)
    assert valid.tolist() == [S.RAW_VALID[w] for w in names] == [1, 1, 0, 0, 1, 1, 1]
    # b: exactly two events vote, the first into bin 0 alone and the last into bin C - 1 alone, each with its signed polarity
    assert int((grids[1] != 0).sum()) == 2 and (grids[1].abs().amax(dim=(1, 2)) == torch.tensor([1.0, 0, 0, 0, 1.0]).cuda()).all()
    _, valid = check_windows(store, [win[w] for w in "efg"], None)
    assert valid.tolist() == [1, 1, 1]
    order = [4, 6, 2, 0, 5, 3, 1]
    _, valid = check_windows(store, [ranges[i] for i in order], S.ROI)
    assert valid.tolist() == [S.RAW_VALID[names[i]] for i in order]


def test_three_hundred_small_windows_and_one_alone():
    store = store_of(False)
    small = S.small_windows()
    _, valid = check_windows(store, small, S.ROI)
    assert 0 < int(valid.sum()) < len(small)
    check_windows(store, [S.raw_recording()[1]["b"]], S.ROI)


def test_long_window_normalised():
    store = store_of(False)
    e = S.raw_recording()[1]["e"]
    x0, x1, y0, y1 = S.ROI
    for roi in (None, dict(xmin=x0, xmax=x1, ymin=y0, ymax=y1)):
        plain, ok = store.voxels([e], S.N_BINS, S.SENSOR, roi=roi, signed=False)   # one sign: nothing cancels
        normed, ok_n = store.voxels([e], S.N_BINS, S.SENSOR, roi=roi, signed=False, normalize=True)
        assert ok.tolist() == ok_n.tolist() == [1]
        same_as_normalised_own_grid(normed[0], plain[0], f"voxels(normalize=True), roi={roi is not None}")
