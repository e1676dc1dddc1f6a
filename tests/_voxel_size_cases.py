"""Seeded inputs at the sizes where the kernels of csrc/event_voxel.hip take another path, shared by tests/test_voxel_size_cases.py
(which pins their make-up on the CPU) and tests/test_gpu_voxel_sizes.py (which runs the kernels on them).  The thresholds:

    norm_reduce_kernel    min(ceil(n / 256), 256) workgroups: a lane folds a second voxel beyond 65 536 voxels
    norm_map_kernel       at most 1024 workgroups: its stride loop starts beyond 262 144 voxels
    volume_range_kernel   at most 2048 workgroups: a lane takes a second event beyond 524 288 events
    raw_bounds_kernel     the ROI scans from either end advance in steps of 256 events

Every builder is a pure function of its arguments; nothing here touches the GPU.
"""
import numpy as np

BLOCK = 256
REDUCE_STRIDE = 256 * BLOCK          # voxels one trip of norm_reduce_kernel covers
MAP_STRIDE = 1024 * BLOCK            # ... of norm_map_kernel
RANGE_STRIDE = 2048 * BLOCK          # events one trip of volume_range_kernel covers

# ------------------------------------------------------------------------------------------------ 1. normaliser
NORM_SHAPES = ((3, 151, 173), (5, 241, 319))      # 78 369 voxels: the reduce strides, the map does not; 384 395: both stride
NORM_VARIANTS = ("drawn", "plus1e6", "minus1e6")
NORM_DRAWS = (0, 1)                                 # two draws x three variants: the six grids of a shape's batch
_OFFSET = {"drawn": 0.0, "plus1e6": 1e6, "minus1e6": -1e6}


def norm_grid(shape, variant, draw=0):
    """float64 ``shape``: uniform in [-3, 3] with about 30 % exact zeros; the variants add +-1e6 to every non-zero voxel, so the
    three grids of a draw share one non-zero mask."""
    rs = np.random.RandomState(4400 + 10 * NORM_SHAPES.index(tuple(shape)) + draw)
    v = rs.uniform(-3.0, 3.0, shape)
    v[rs.rand(*shape) < 0.3] = 0.0
    return np.where(v != 0, v + _OFFSET[variant], 0.0)


def norm_cases():
    return [(s, v, d) for s in NORM_SHAPES for d in NORM_DRAWS for v in NORM_VARIANTS]


# the end-to-end grid: more events than one trip of the range kernel and than 2048 workgroups of the vote kernel
VOXEL_EVENTS = RANGE_STRIDE + 300
VOXEL_SHAPE = NORM_SHAPES[1]


def voxel_events():
    """(x, y, pol, t) float64 [524 588]: fractional pixels from inside (-1, 0) to beyond the last pixel, one polarity (nothing
    cancels, so the non-zero mask does not depend on the order of the votes), times sorted."""
    rs = np.random.RandomState(4421)
    C, H, W = VOXEL_SHAPE
    n = VOXEL_EVENTS
    x, y = rs.uniform(-0.9, W - 0.1, n), rs.uniform(-0.9, H - 0.1, n)
    t = np.sort(rs.uniform(0.0, 1.0, n))
    return x, y, np.ones(n), t


# ------------------------------------------------------------------------------------------------ 2. discretised volume
VOLUME_EVENTS = RANGE_STRIDE + 300     # the second trip holds 300 events: four full waves and 44 lanes of a fifth
VOLUME_SIZE = (10, 24, 32)
NAN_INDEX = RANGE_STRIDE + 12          # 524 300
HEAD = 7
# case -> (where the smallest time sits, where the largest): "tail" is an index >= RANGE_STRIDE, "head" is index HEAD
VOLUME_CASES = {"both_tail": ("tail", "tail"), "min_tail_max_head": ("tail", "head"), "max_tail_min_head": ("head", "tail"),
                "all_negative": ("tail", "tail"), "signed_zeros": ("tail", "tail")}


def volume_events(case, dtype=np.float64):
    """[n, 4] = (x, y, t, p) in ``dtype``: unsorted times uniform in [-2.99, 4.99) with the two extremes, -2.9973 and 4.9981, set
    where VOLUME_CASES says -- apart from them, so that they stay the only smallest and largest time in float32 too.
    "all_negative": everything 5.5 lower; "signed_zeros": uniform in [0.01, 4.99) with -0.0 (in the tail) and +0.0 (at index 3) as
    the two smallest."""
    rs = np.random.RandomState(4430 + list(VOLUME_CASES).index(case))
    n = VOLUME_EVENTS
    T, X, Y = VOLUME_SIZE
    ev = np.empty((n, 4))
    ev[:, 0], ev[:, 1] = rs.randint(0, X, n), rs.randint(0, Y, n)
    ev[:, 3] = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    t = rs.uniform(0.01 if case == "signed_zeros" else -2.99, 4.99, n)
    tail = iter((RANGE_STRIDE + 5, n - 1))          # a lane of the second trip's first wave, and the last event of all
    where_min, where_max = VOLUME_CASES[case]
    i_min = HEAD if where_min == "head" else next(tail)
    i_max = HEAD if where_max == "head" else next(tail)
    t[i_min], t[i_max] = -2.9973, 4.9981
    if case == "all_negative":
        t -= 5.5
    if case == "signed_zeros":
        t[i_min], t[3] = -0.0, 0.0
    ev[:, 2] = t
    return ev.astype(dtype)


def extremes(ev):
    """(indices of the smallest time, indices of the largest) -- every index that holds it; -0.0 == +0.0 here."""
    t = ev[:, 2]
    return np.flatnonzero(t == t.min()), np.flatnonzero(t == t.max())


# ------------------------------------------------------------------------------------------------ 3. windows of raw columns
SENSOR = (24, 32)
ROI = (4, 20, 6, 26)                   # rows [4, 20), columns [6, 26): crop_event's x0, x1, y0, y1
N_BINS = 5
RAW_VALID = {"a": 1, "b": 1, "c": 0, "d": 0, "e": 1, "f": 1, "g": 1}
_cache = {}


def raw_recording():
    """-> (columns {"x" = column int16, "y" = row int16, "t" int32 ticks, "p" bool}, windows {name: (begin, end)}).

    D = events outside ROI, K = events inside, M = uniform over the sensor (about 42 % inside); t strictly increasing.
        a   700 D, 2000 M (the first and the last of them K), 700 D     either scan takes three steps
        b   600 D, K, 1000 D, K, 600 D                                  exactly two events vote
        c   800 D, K, 699 D                                             one kept event, at position 800: no span
        d   1000 D                                                      nothing kept
        e   300 000 M                                                   sizes the vote grid of every call it is in
        f   3 K        g   2 K                                          tiny windows beside e
    """
    if "raw" in _cache:
        return _cache["raw"]
    rs = np.random.RandomState(4440)
    x0, x1, y0, y1 = ROI
    H, W = SENSOR

    def mixed(n):
        return rs.randint(0, H, n), rs.randint(0, W, n)

    def kept(n):
        return rs.randint(x0, x1, n), rs.randint(y0, y1, n)

    def dropped(n):                                 # uniform, and whatever fell inside moved to a row above or below ROI
        row, col = mixed(n)
        inside = (row >= x0) & (row < x1) & (col >= y0) & (col < y1)
        outer = np.concatenate([np.arange(0, x0), np.arange(x1, H)])
        row[inside] = outer[rs.randint(0, len(outer), int(inside.sum()))]
        return row, col

    def mixed_with_kept_ends(n):
        row, col = mixed(n)
        (row[0], row[-1]), (col[0], col[-1]) = kept(2)
        return row, col

    layout = {"a": [dropped(700), mixed_with_kept_ends(2000), dropped(700)],
              "b": [dropped(600), kept(1), dropped(1000), kept(1), dropped(600)],
              "c": [dropped(800), kept(1), dropped(699)],
              "d": [dropped(1000)],
              "e": [mixed(300_000)],
              "f": [kept(3)],
              "g": [kept(2)]}
    rows, cols, windows, at = [], [], {}, 0
    for name, parts in layout.items():
        n = sum(len(r) for r, _ in parts)
        windows[name] = (at, at + n)
        at += n
        rows += [r for r, _ in parts]
        cols += [c for _, c in parts]
    row, col = np.concatenate(rows), np.concatenate(cols)
    columns = {"x": col.astype(np.int16), "y": row.astype(np.int16),
               "t": (1_000_000 + np.cumsum(rs.randint(1, 20, at))).astype(np.int32), "p": rs.randint(0, 2, at).astype(bool)}
    _cache["raw"] = columns, windows
    return _cache["raw"]


def small_windows():
    """300 windows of 5 .. 40 events inside e, overlapping and in no order."""
    rs = np.random.RandomState(4441)
    e0, e1 = raw_recording()[1]["e"]
    begin = rs.randint(e0, e1 - 40, 300)
    return [(int(b), int(b + n)) for b, n in zip(begin, rs.randint(5, 41, 300))]


def kept_events(store, window, roi=ROI):
    """The reference-format events of ``window`` that ``roi`` keeps (all of them with ``roi=None``), as ``crop_event`` leaves them."""
    from event_based_bos_amd.utils import crop_event

    ev = store.load_event(*window)
    return ev if roi is None else crop_event(ev, *roi)


def expect_valid(ev):
    return int(len(ev) >= 2 and ev[-1, 2] != ev[0, 2])
