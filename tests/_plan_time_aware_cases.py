"""Shared cases of tests/test_gpu_plan_time_aware.py: a small raw recording (sensor columns), the six ranges of the batch and the
comparison of two binned time-aware plans up to the order of the events of one source pixel.

Shapes: about 60 000 events with sorted ticks on 37 x 70 (plan tile (32, 32): tiles overhang both axes) or 64 x 96 (tile (64, 64)),
some columns / rows outside the image on either side, 3 000 more events on one source pixel with times over the whole recording."""
import numpy as np
import torch

GEOMETRIES = {"37x70": ((37, 70), (32, 32)), "64x96": ((64, 96), (64, 64))}
N_BASE, HOT_EXTRA, HOT_PIXEL = 57_000, 3_000, (17, 33)
TICKS_PER_SECOND = 1e6
ROI, REMOVE = (3, 30, 5, 60), (10, 20, 20, 40)          # rows [xmin, xmax) x columns [ymin, ymax)
RECTS = {"none": (None, None), "roi": (ROI, None), "remove": (None, REMOVE), "both": (ROI, REMOVE)}
INSIDE = (5, 10)                                          # a pixel inside the image and ROI, outside REMOVE, at both geometries
_cache = {}


def dev():
    return torch.device("cuda:0")


def raw_columns(geometry: str, seed: int = 7):
    """(col int16, row int16, ticks int64, pol uint8) as numpy, ticks sorted."""
    key = ("raw", geometry, seed)
    if key not in _cache:
        (H, W), _ = GEOMETRIES[geometry]
        rs = np.random.RandomState(seed)
        n = N_BASE + HOT_EXTRA
        col = rs.randint(-3, W + 3, n).astype(np.int16)      # some events left of / right of the image
        row = rs.randint(-2, H + 2, n).astype(np.int16)      # ... above / below it
        hot = rs.choice(n, HOT_EXTRA, replace=False)          # the stuck pixel fires over the whole recording: every bin of every window
        row[hot], col[hot] = HOT_PIXEL
        ticks = np.sort(rs.randint(1_000_000, 1_600_000, n)).astype(np.int64)
        pol = rs.randint(0, 2, n).astype(np.uint8)
        # the events the degenerate ranges hold, and the ends of the 20 000-event range, lie inside the image and pass both rectangles
        for i in (200, 300, 301, 1000, 20_999):
            row[i], col[i] = INSIDE
        ticks[301] = ticks[300]
        assert (np.diff(ticks) >= 0).all() and ticks[20_999] > ticks[1000]
        assert (col < 0).any() and (col >= W).any() and (row < 0).any() and (row >= H).any()
        _cache[key] = (col, row, ticks, pol)
    return _cache[key]


def ranges_of(n: int):
    """empty, one event, two events with equal ticks, 20 000 events, a range overlapping the previous one, the whole store"""
    return [(100, 100), (200, 201), (300, 302), (1000, 21_000), (15_000, 30_000), (0, n)]


def device_columns(geometry: str, t64: bool):
    col, row, ticks, pol = raw_columns(geometry)
    t = ticks if t64 else ticks.astype(np.int32)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in (col, row, t, pol))


def keep_mask(col, row, roi, remove):
    """numpy restatement of evaluation._keep_mask"""
    keep = np.ones(len(col), dtype=bool)
    if roi is not None:
        keep &= (row >= roi[0]) & (row < roi[1]) & (col >= roi[2]) & (col < roi[3])
    if remove is not None:
        keep &= ~((row >= remove[0]) & (row < remove[1]) & (col >= remove[2]) & (col < remove[3]))
    return keep


def canonical(plan, source_index=None):
    """A binned plan's streams on the host with every source pixel's run ordered by the events' source index:
    {src, x, y, dt (int32 bit patterns), bins}.  ``source_index`` (numpy, optional): maps ``plan.perm`` to the index space compared in."""
    n = int(plan.n)
    ko = plan.key_offsets.cpu().numpy().astype(np.int64)
    assert ko[0] == 0 and ko[-1] == n and (np.diff(ko) >= 0).all()
    keys = np.repeat(np.arange(len(ko) - 1), np.diff(ko))
    src = plan.perm[:n].cpu().numpy().astype(np.int64)
    if source_index is not None:
        src = source_index[src]
    order = np.lexsort((src, keys))
    return {"src": src[order], "x": plan.x[:n].cpu().numpy()[order], "y": plan.y[:n].cpu().numpy()[order],
            "dt": plan.dt[:n].contiguous().view(torch.int32).cpu().numpy()[order], "bins": plan.bins[:n].cpu().numpy()[order]}


def same_plan(a: dict, b: dict) -> bool:
    return all(np.array_equal(a[k], b[k]) for k in ("src", "x", "y", "dt", "bins"))
