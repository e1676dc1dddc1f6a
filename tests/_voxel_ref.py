"""numpy restatement of the reference's two time-resolved event representations (src/utils/event_utils.py:291-440), what the
GPU tests compare the kernels of csrc/event_voxel.hip with.  tests/test_voxel.py pins it to tests/golden/golden_voxel.npz, the
arrays the reference itself produced, exactly: both add the votes of a voxel sequentially and in one order (the reference's
``put_(accumulate=True)`` on the CPU walks its index array front to back, as ``np.add.at`` does).

Besides the grid, both functions return per voxel the number of contributions ``k`` and the sum of their magnitudes ``sabs``
(float64): two summation orders of the same k addends differ by at most ``2 k u sabs`` (``error_bound``; every partial sum is
bounded by sabs and each of the k - 1 additions of either order rounds once, relative u).  ``within_bound`` is that check, shared
by the GPU tests.
"""
import math

import numpy as np


def error_bound(k, sabs, u=2.0 ** -53):
    return 2.0 * k * u * sabs


def within_bound(got, ref, u=2.0 ** -53):
    """``got`` (a numpy array or a torch tensor on any device) against ``ref`` = (grid, k, sabs) of a restatement below."""
    want, k, sabs = ref
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    assert got.shape == want.shape and got.dtype == want.dtype
    err, bound = np.abs(got.astype(np.float64) - want.astype(np.float64)), error_bound(k, sabs, u)
    worst = (err / np.where(bound > 0, bound, 1.0)).max()
    print(f"max |gpu - ref| {err.max():.3e}, worst share of the bound {worst:.3f}, {int((k == 0).sum())} voxels without a vote")
    assert (got[k == 0] == 0).all()
    assert (err <= bound).all(), (float(err.max()), int((err > bound).sum()))


def create_event_voxel(x, y, pol, time, voxel_shape, normalize=False):
    """-> (grid float64 [C, H, W], k int64 [C, H, W], sabs float64 [C, H, W]); k and sabs describe the votes before normalisation."""
    x, y, pol, time = (np.asarray(a, dtype=np.float64) for a in (x, y, pol, time))
    assert x.shape == y.shape == pol.shape == time.shape and x.ndim == 1
    C, H, W = voxel_shape
    grid, k, sabs = np.zeros(C * H * W), np.zeros(C * H * W, dtype=np.int64), np.zeros(C * H * W)
    with np.errstate(all="ignore"):
        t_norm = (C - 1) * (time - time[0]) / (time[-1] - time[0])
        x0, y0, t0 = (np.trunc(a).astype(np.int32) for a in (x, y, t_norm))   # .int(): towards zero
        for xlim in (x0, x0 + 1):
            for ylim in (y0, y0 + 1):
                for tlim in (t0, t0 + 1):
                    mask = (xlim < W) & (xlim >= 0) & (ylim < H) & (ylim >= 0) & (tlim >= 0) & (tlim < C)
                    w = pol * (1 - np.abs(xlim - x)) * (1 - np.abs(ylim - y)) * (1 - np.abs(tlim - t_norm))
                    index = H * W * tlim.astype(np.int64) + W * ylim.astype(np.int64) + xlim.astype(np.int64)
                    np.add.at(grid, index[mask], w[mask])
                    np.add.at(k, index[mask], 1)
                    np.add.at(sabs, index[mask], np.abs(w[mask]))
    grid = grid.reshape(C, H, W)
    if normalize:
        grid = normalize_voxel(grid)
    return grid, k.reshape(C, H, W), sabs.reshape(C, H, W)


def normalize_voxel(grid):
    """:356-364 on a copy: the non-zero voxels to (v - mean) / std (unbiased), v - mean when std is not > 0."""
    grid = np.array(grid, dtype=np.float64)
    mask = grid != 0
    if mask.sum() > 0:
        mean = grid[mask].mean()
        with np.errstate(all="ignore"):
            std = grid[mask].std(ddof=1) if mask.sum() > 1 else np.nan
        grid[mask] = (grid[mask] - mean) / std if std > 0 else grid[mask] - mean
    return grid


def normalize_exact(grid):
    """``normalize_voxel`` with the moments summed exactly: the mean from ``math.fsum`` (one rounding, and one more in the
    division), m2 as ``math.fsum`` of the squared deviations from that mean, std = sqrt(m2 / (k - 1)), then the reference's map.
    What the normaliser is held to where the order of a plain sum would matter: 10^5 voxels, or a mean far from zero."""
    grid = np.array(grid, dtype=np.float64)
    mask = grid != 0
    v = grid[mask]
    if v.size == 0:
        return grid
    mean = math.fsum(v) / v.size
    d = v - mean
    std = math.sqrt(math.fsum(d * d) / (v.size - 1)) if v.size > 1 else math.nan
    grid[mask] = d / std if std > 0 else d
    return grid


def normalize_bound(grid, u=2.0 ** -53):
    """The per-voxel bar of the GPU normaliser against ``normalize_exact``: 64 u max|v| / std.  A lane's Welford pass folds at most
    6 voxels and 8 + 8 Chan merges follow (a workgroup's tree, then the tree over the partials); each of those ~22 steps rounds
    once, relative u, a quantity no larger than max|v|; the subtraction and the division of the map add two; doubled, 64.  The
    error of the mean is what this measures: it shifts every voxel by (error / std)."""
    v = np.asarray(grid, dtype=np.float64)
    v = v[v != 0]
    d = v - math.fsum(v) / v.size
    return 64.0 * u * np.abs(v).max() / math.sqrt(math.fsum(d * d) / (v.size - 1))


def generate_discretized_event_volume(events, vol_size):
    """-> (volume [T, X, Y] in the events' dtype, k int64, sabs float64).  All arithmetic in the events' dtype, as torch's;
    ``(nb - 1) / (t_max - t_min)`` on a tensor is torch's ``__rdiv__``: ``reciprocal() * (nb - 1)``."""
    events = np.asarray(events)
    dt = events.dtype.type
    T, X, Y = vol_size
    nb = T // 2
    vol, k, sabs = np.zeros(T * X * Y, dtype=dt), np.zeros(T * X * Y, dtype=np.int64), np.zeros(T * X * Y)
    x, y, t, p = events[:, 0].astype(np.int64), events[:, 1].astype(np.int64), events[:, 2], events[:, 3]
    t_min, t_max = t.min(), t.max()
    t_scaled = (t - t_min) * ((dt(1) / (t_max - t_min)) * dt(nb - 1))
    x_fl = np.floor(t_scaled + dt(1e-8))
    x_ce = np.ceil(t_scaled - dt(1e-8))
    dx_ce = t_scaled - x_fl
    dx_fl = (np.floor(t_scaled) + dt(1)) - t_scaled
    for tb, w in ((x_fl.astype(np.int64), dx_fl), (x_ce.astype(np.int64), dx_ce)):
        assert (x >= 0).all() and (x < X).all() and (y >= 0).all() and (y < Y).all() and (tb >= 0).all() and (tb < nb).all()
        inds = (X * Y) * (tb + np.where(p < 0, nb, 0)) + Y * x + y
        np.add.at(vol, inds, w)
        np.add.at(k, inds, 1)
        np.add.at(sabs, inds, np.abs(w.astype(np.float64)))
    return vol.reshape(T, X, Y), k.reshape(T, X, Y), sabs.reshape(T, X, Y)


def voxel_of_events(events, n_bins, image_shape, signed=True, origin=(0, 0)):
    """The grid ``RawEventStore.voxels`` stands for, from reference-format events [n, 4] = (row, col, t, p in {0, 1}): x = column,
    y = row, both shifted by ``origin`` = (row, column) of a crop."""
    pol = 2.0 * events[:, 3] - 1.0 if signed else events[:, 3]
    H, W = image_shape
    return create_event_voxel(events[:, 1] - origin[1], events[:, 0] - origin[0], pol, events[:, 2], (n_bins, H, W))
