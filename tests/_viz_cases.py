"""Seeded inputs of the visualizer tests (tests/test_viz.py checks the seeds on the CPU, tests/test_gpu_viz.py runs them)."""
import numpy as np

SHAPES = [(30, 50), (64, 96)]     # no multiple of any tile with odd halo cases; a multiple of the 4-pixel lane and of the close's tile


def flows(shape, b):
    """(pred, gt) [2, H, W] float64 of window b: smooth fields of a few pixels plus noise; pred has a block of exact zeros."""
    H, W = shape
    rs = np.random.RandomState(1000 + 17 * b + H)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    pred = np.stack([2.5 * np.sin(yy / 7.0 + b) + 0.3 * rs.randn(H, W), 1.5 * np.cos(xx / 9.0) + 0.3 * rs.randn(H, W)])
    gt = np.stack([2.0 * np.sin(yy / 6.0) + 0.2 * rs.randn(H, W), 3.0 * np.cos(xx / 11.0 + b) + 0.2 * rs.randn(H, W)])
    pred[:, H // 3:H // 3 + 5, W // 4:W // 4 + 7] = 0.0
    return pred, gt


def bad_flow(shape):
    """pred of window 0 with a NaN component, a +inf component (beside an exact zero) and its block of zeros."""
    f = flows(shape, 0)[0].copy()
    f[0, 3, 4] = np.nan
    f[1, 5, 6], f[0, 5, 6] = np.inf, 0.0
    return f


def events(shape, b, n=900):
    """(unfiltered [n, 4], filtered subset) on integer pixels, polarity 0 / 1; pixels that saturate the grey pictures; every corner."""
    H, W = shape
    rs = np.random.RandomState(2000 + b + W)
    ev = np.stack([rs.randint(0, H, n), rs.randint(0, W, n), np.sort(rs.uniform(0, 0.01, n)), rs.randint(0, 2, n)], axis=1).astype(np.float64)
    ev[:9, :2], ev[:9, 3] = (10, 20), 1
    ev[9:18, :2], ev[9:18, 3] = (15, 30), 0
    ev[18, :2], ev[19, :2], ev[20, :2], ev[21, :2] = (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)
    keep = (ev[:, 0] >= 4) & (ev[:, 0] < H - 4) & (ev[:, 1] >= 6) & (ev[:, 1] < W - 6)
    return ev, ev[keep][::2]


def counts(ev, shape):
    """[2, H, W]: events per pixel with polarity 1 / 0."""
    out = np.zeros((2,) + tuple(shape))
    r, c, p = ev[:, 0].astype(int), ev[:, 1].astype(int), ev[:, 3] > 0
    np.add.at(out[0], (r[p], c[p]), 1)
    np.add.at(out[1], (r[~p], c[~p]), 1)
    return out


def masks(shape):
    """Random masks of density 0.02, 0.3 and 0.9, one with every corner and edge set, an empty and a full one."""
    H, W = shape
    rs = np.random.RandomState(77 + H)
    out = [(rs.rand(H, W) < d).astype(np.uint8) for d in (0.02, 0.3, 0.9)]
    edge = np.zeros((H, W), dtype=np.uint8)
    edge[0, 0] = edge[0, -1] = edge[-1, 0] = edge[-1, -1] = 1
    edge[0, W // 2] = edge[-1, W // 3] = edge[H // 2, 0] = edge[H // 3, -1] = 1
    edge[0, 2] = edge[2, 0] = edge[-1, -3] = edge[-3, -1] = 1      # gaps next to the border close against it
    out += [edge, np.zeros((H, W), dtype=np.uint8), np.ones((H, W), dtype=np.uint8)]
    return np.stack(out)
