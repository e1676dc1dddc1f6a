"""Shared cases of tests/test_gpu_bwd_loop_boundaries.py (pinned on the CPU by tests/test_bwd_loop_cases.py): windows that put chosen
numbers of events into the four tiles of a 2 x 2-tile image, for the event loop of the tile-private backward kernel
(csrc/iwe_tile_core.h: bwd_compact_slice, bwd_sweeps_mode, bwd_lean_sweeps, the set-up around BwdPre).

That loop takes chunks of 64 groups of 4 events; a workgroup has 16 waves, chunks 0 .. 31 are pre-assigned (two per wave) and every
chunk past 8192 events of a work item is drawn from an LDS counter (ChunkQueue).  The sets, events per tile:

    a   (0, 1, 3, 4)                     an empty tile, a padded group, an exact group
    b   (255, 256, 257, 3842)            around one chunk; a partial chunk on wave 15
    c   (4096, 4100, 8191, 8192)         16, 17 and 32 chunks: the last sizes at which no draw from the queue is live
    d   (8193, 8449, 8705, 8961)         33 .. 36 chunks: one to four waves take a third chunk (the third register set of the
                                         fixed-point sweep's rotation); the last chunk holds ONE group with ONE live event
    e   (12289, 16385, 20481, 24577)     49, 65, 81, 97 chunks: 3 to 7 chunks per wave

WHICH wave draws which chunk is decided at run time by the order in which the waves reach the counter, so no seed pins down the
exit a given wave leaves the three-step rotation by (a wave that took n chunks leaves in front of place n mod 3: first, second,
third).  What the sets do pin down is how many chunks the 16 waves of a tile share: the four tiles of set e hold 49, 65, 81 and 97
chunks, 3.06, 4.06, 5.06 and 6.06 per wave and one more than a multiple of 16, so the waves of one tile cannot all take the same
number, and with any near-even sharing they end after 3 | 4, 4 | 5, 5 | 6 and 6 | 7 chunks: over the four tiles every exit of the
rotation -- the second place, the third, and the first again -- is taken on every run, whichever waves take it.

Other inputs, all seeded: a dense flow uniform in +-5 px (with normalised |dt| <= 1 nothing leaves the smallest built halo, 8); an
upstream image uniform in +-1 per pixel, fixed, so that the backward loop is tested apart from the forward pass; flow overrides for
the special cases (a row of 40 px through a tile, a field of 30 px against halo 8).  Helpers count chunks per tile, events per source
pixel, and -- with the float64 oracle's warp -- the events whose taps leave the tile + halo window, and where they sit in the plan.
"""
import numpy as np
import torch

from oracle import ebos_oracle as O

GEOMETRIES = [((90, 160), (45, 80)), ((128, 128), (64, 64)), ((64, 64), (32, 32))]   # (image, tile): 2 x 2 tiles
SETS = {
    "a": (0, 1, 3, 4),
    "b": (255, 256, 257, 4 * 64 * 15 + 2),
    "c": (4096, 4100, 8191, 8192),
    "d": (8193, 8449, 8705, 8961),
    "e": (12289, 16385, 20481, 24577),
}
CHUNKS = {"a": (0, 1, 1, 1), "b": (1, 1, 2, 16), "c": (16, 17, 32, 32), "d": (33, 34, 35, 36), "e": (49, 65, 81, 97)}
# the loop of plans that are not lean (per-event weights, the (x, y, dt) format) strides statically by kBlock = 1024 groups
NONLEAN_SETS = {"f": (4092, 4096, 4100, 8192), "g": (8196, 4092, 4096, 4100)}   # 1023, 1024, 1025, 2048 | 2049 groups
GROUP, WAVE, WAVES, BLOCK = 4, 64, 16, 1024           # events per group, groups per chunk, waves per workgroup, kBlock
PRE_ASSIGNED = 2 * WAVES                               # chunks 0 .. 31
HOT_MIN, FX_BITS, HALO_MIN = 1024, 21, 8               # bwd_fx_unit: f64 from the start | bits per event | the smallest built halo
# the built (tile_h, tile_w, halo) of the slab family (csrc/tile_configs.h) that fit a geometry above; the GPU test asserts that
# _hip.slab_configs() restricted to these tiles is this list
TRIPLES = [(45, 80, 32), (64, 64, 32), (32, 32, 32), (64, 64, 16), (45, 80, 16), (32, 32, 16), (32, 32, 8)]
MAIN = (45, 80, 32)
FLOW_AMP, SPILL_ROW_FLOW, BIG_FLOW_AMP, SPIKE = 5.0, 40.0, 30.0, 1e6
SPEC_FLOW_AMP = 2.5                                    # a field the 4 px speculative window of halo="auto" holds
HOT = (3, 1500)                                        # 1500 of tile 3's events on one pixel
HOT_WRAP = (3, 5000)                                   # forward: 5000 x 2^20 does not fit the 32-bit field of the LDS image
BATCH_TILE3 = (0, 8193, 1, 24577, 0)                   # persistent batch: events of tile 3 in five consecutive windows
BATCH_OTHERS = (300, 5000, 1000)                       # ... and of tiles 0 .. 2 in each of them
N_CU_MODEL, PART_FIXED_EVENTS = 256, 8192              # ebos_plan_parts on an MI355X, few tiles (event_plan.part_fixed_events)

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def geometry_of(tile):
    return next(g for g in GEOMETRIES if g[1] == tuple(tile))


def chunks_of(n):
    """Chunks of a work item of n events: ceil(ceil(n / 4) / 64)."""
    return -(-(-(-n // GROUP)) // WAVE)


def events(size, tile, counts, seed, hot=None, fractional=False):
    """[n, 4] float64 events (row, column, t, p), times sorted and covering [0, 0.5]: counts[k] events in tile k of the 2 x 2 tiles,
    uniform over the tile's pixels (the scheme of tests/test_dense_loop_two_groups.py); hot = (k, m): m of tile k's events sit on ONE
    pixel; fractional: source coordinates with a fraction of 1/4 .. 3/4 px (such a plan keeps the (x, y, dt) format)."""
    (h, w), (th, tw) = size, tile
    assert (h, w) == (2 * th, 2 * tw)
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    for k, n in enumerate(counts):
        r0, c0 = (k // 2) * th, (k % 2) * tw
        r, c = rs.randint(0, th, n) + r0, rs.randint(0, tw, n) + c0
        if hot is not None and hot[0] == k:
            r[: hot[1]], c[: hot[1]] = r0 + th // 2, c0 + tw // 3
        rows.append(r), cols.append(c)
    rows, cols = np.concatenate(rows).astype(np.float64), np.concatenate(cols).astype(np.float64)
    order = rs.permutation(rows.size)
    t = np.sort(rs.uniform(0.0, 0.5, rows.size))
    if t.size:
        t[0], t[-1] = 0.0, 0.5
    if fractional:
        rows, cols = rows + rs.randint(1, 4, rows.size) / 4.0, cols + rs.randint(1, 4, rows.size) / 4.0
    return np.stack([rows[order], cols[order], t, rs.randint(0, 2, rows.size)], axis=1).astype(np.float64)


def window(tile, name, hot=None, fractional=False):
    """The window of set ``name`` on the geometry of ``tile``: one seed per (set, geometry)."""
    size, tile = geometry_of(tile)
    counts = SETS[name] if name in SETS else NONLEAN_SETS[name]
    seed = 100 * GEOMETRIES.index((size, tile)) + ord(name[0]) + (7 if hot else 0) + (13 if fractional else 0)
    return cached(("ev", tile, name, hot, fractional), lambda: events(size, tile, counts, seed, hot, fractional))


def batch_windows(tile=(45, 80)):
    """Five windows for one persistent batch: tile 3 goes 0 -> 8193 -> 1 -> 24577 -> 0 events, the other tiles stay."""
    size, tile = geometry_of(tile)
    return cached(("batch", tile), lambda: [events(size, tile, BATCH_OTHERS + (n,), 300 + k) for k, n in enumerate(BATCH_TILE3)])


def tile_index(ev, size, tile):
    return (ev[:, 0].astype(np.int64) // tile[0]) * 2 + ev[:, 1].astype(np.int64) // tile[1]


def tile_counts(ev, size, tile):
    return tuple(int(v) for v in np.bincount(tile_index(ev, size, tile), minlength=4))


def pixel_counts(ev, size):
    """Events per source pixel [H, W]."""
    lin = ev[:, 0].astype(np.int64) * size[1] + ev[:, 1].astype(np.int64)
    return np.bincount(lin, minlength=size[0] * size[1]).reshape(size)


def tile_slices(size, tile):
    return [(slice((k // 2) * tile[0], (k // 2 + 1) * tile[0]), slice((k % 2) * tile[1], (k % 2 + 1) * tile[1])) for k in range(4)]


def flow(size, seed=5, amp=FLOW_AMP):
    return cached(("flow", tuple(size), seed, amp), lambda: np.random.RandomState(seed).uniform(-amp, amp, (2,) + tuple(size)))


def upstream(size, seed=9):
    return cached(("up", tuple(size), seed), lambda: np.random.RandomState(seed).uniform(-1.0, 1.0, tuple(size)))


def weights(n, seed=15):
    """Per-event weights in input order, in [0.5, 1.5]."""
    return cached(("w", n, seed), lambda: np.random.RandomState(seed).uniform(0.5, 1.5, n))


# ---------------------------------------------------------------------------------------------- flow overrides
def spill_row(size, tile, k=3):
    """The pixel row through the middle of tile k."""
    return (k // 2) * tile[0] + tile[0] // 2


def row_flow(size, tile, k=3):
    """``flow(size)`` with SPILL_ROW_FLOW px along the columns on one pixel row through the middle of tile k (and of its neighbour in
    the tile row): the events of that row move left by up to 40 px.  The row lies in the second half of the tile's plan order (chunks
    >= 32 of the 24 577-event tile), and from a right-hand tile the events of its leftmost columns leave a window of halo 32 --
    those of most columns one of halo 8 -- and stay inside the image.  (Up or down, no row of the second half of a 45-row tile
    leaves a 32 px halo with 40 px and stays inside the image.)"""
    fl = flow(size).copy()
    fl[1, spill_row(size, tile, k), :] = SPILL_ROW_FLOW
    return fl


def big_flow(size, seed=6):
    """A field of +-30 px: against halo 8 most events leave their window."""
    return flow(size, seed, BIG_FLOW_AMP)


AIM_ROWS, AIM_COLS, AIM_DT = (11, 14), (0, 9), 0.85   # pixels of tile 3 (rows / columns inside the tile) whose events pass the spike


def aimed_flow(size, tile):
    """``big_flow`` with a block of tile 3's pixels aimed at the upstream spike: their events pass it at normalised dt = 0.85, from
    rows of the tile that lie past its first 8192 events in plan order, with |flow| < 30 px."""
    fl = big_flow(size).copy()
    (sr, sc), (r0, c0) = spike_pixel(tile), (tile[0], tile[1])
    for r in range(r0 + AIM_ROWS[0], r0 + AIM_ROWS[1]):
        for c in range(c0 + AIM_COLS[0], c0 + AIM_COLS[1]):
            fl[0, r, c], fl[1, r, c] = (r - sr - 0.3) / AIM_DT, (c - sc - 0.3) / AIM_DT
    return fl


def reach_flow(size, tile, k=3, px=20.0):
    """``flow(size)`` with |flow| = px on the whole of tile k: what a run-time window (halo="auto") sized for 5 px does not hold."""
    fl = flow(size).copy()
    rs, cs = tile_slices(size, tile)[k]
    fl[0, rs, cs], fl[1, rs, cs] = px, -px
    return fl


def spike_pixel(tile):
    """Where the upstream spike of the f64-redo case sits: in tile 0, 4 px outside the halo-8 windows of the other three tiles."""
    return (tile[0] - HALO_MIN - 4, tile[1] - HALO_MIN - 4)


def spike_upstream(size, tile):
    up = upstream(size).copy()
    up[spike_pixel(tile)] = SPIKE
    return up


# ---------------------------------------------------------------------------------------------- the oracle's warp
def warped(ev, fl, direction="first"):
    """(x', y') of the float64 oracle's dense-flow warp, normalised time."""
    with torch.no_grad():
        return O.warp_dense_torch(torch.from_numpy(ev), torch.from_numpy(fl), direction, True).numpy()[:, :2]


def beyond_window(ev, fl, size, tile, halo, direction="first"):
    """bool [n]: the event's top-left tap, by the oracle's warp, lies outside rows / columns [0, L - 1) of the tile + halo window of
    its source tile (the backward's spill sweep takes it) and inside the image (it contributes)."""
    xy = warped(ev, fl, direction)
    top = np.floor(xy)
    out = np.zeros(len(ev), dtype=bool)
    for axis, t in ((0, tile[0]), (1, tile[1])):
        cell = top[:, axis] - ((ev[:, axis].astype(np.int64) // t) * t - halo)
        out |= (cell < 0) | (cell >= t + 2 * halo - 1)
    inside = (top[:, 0] >= 0) & (top[:, 0] < size[0] - 1) & (top[:, 1] >= 0) & (top[:, 1] < size[1] - 1)
    return out & inside


def touches(ev, fl, pixel, direction="first"):
    """bool [n]: one of the event's four taps is ``pixel``."""
    top = np.floor(warped(ev, fl, direction))
    return ((top[:, 0] == pixel[0]) | (top[:, 0] + 1 == pixel[0])) & ((top[:, 1] == pixel[1]) | (top[:, 1] + 1 == pixel[1]))


def first_chunk(ev, size, tile):
    """int [n]: the chunk (of its tile's work item, splits = 1) in which the run of the event's source pixel BEGINS -- a plan orders
    a tile's events by source pixel, row-major inside the tile; an event sits in that chunk or a later one."""
    k = tile_index(ev, size, tile)
    pix = (ev[:, 0].astype(np.int64) % tile[0]) * tile[1] + ev[:, 1].astype(np.int64) % tile[1]
    out = np.zeros(len(ev), dtype=np.int64)
    for t in range(4):
        m = k == t
        starts = np.concatenate([[0], np.cumsum(np.bincount(pix[m], minlength=tile[0] * tile[1]))])
        out[m] = starts[pix[m]] // (GROUP * WAVE)
    return out


# ---------------------------------------------------------------------------------------------- the work-item model
def adaptive_parts(counts, n_cu=N_CU_MODEL, fixed=PART_FIXED_EVENTS):
    """Parts per tile of ``ebos_plan_parts`` (csrc/event_plan.hip, plan_parts_body) for tiles of ``counts`` events, in plain Python."""
    n_tiles, n_items, lmax, total = len(counts), 2 * len(counts), max(max(counts), 1), sum(counts)
    items_at = lambda tau: sum(max(1, -(-c // tau)) for c in counts)   # noqa: E731
    lo, hi = 1, lmax
    if (lmax + fixed) * 80 * n_cu <= (total + n_tiles * fixed) * 100 or lmax * 4 < fixed:
        lo = hi
    while lo < hi:
        mid = lo + (hi - lo) // 2
        lo, hi = (lo, mid) if items_at(mid) <= n_items else (mid + 1, hi)
    hi = lmax
    while lo < hi:
        mid = lo + (hi - lo) // 2
        lo, hi = (lo, mid) if (mid + fixed) * n_cu >= total + items_at(mid) * fixed else (mid + 1, hi)
    if (lo + fixed) * 100 > (lmax + fixed) * 80:
        lo = lmax
    return tuple(1 if lo >= lmax else max(1, -(-c // lo)) for c in counts)


# ---------------------------------------------------------------------------------------------- float64 yardstick (ii)
def ref_variance_grad(key, ev, fl, size, omit=False, pad=(0, 0), weight=None):
    """(variance, d variance / d flow [2, H, W]) of the float64 oracle's autograd."""
    def make():
        f = torch.from_numpy(fl).clone().requires_grad_(True)
        w = 1.0 if weight is None else torch.from_numpy(weight)
        v = O.image_variance(O.iwe_dense(torch.from_numpy(ev), f, size, pad=pad, weight=w), omit, direction="maximize")
        v.backward()
        return v.item(), f.grad.numpy()
    return cached(("ref-var", key, omit, tuple(pad), weight is not None), make)


def ref_upstream_grad(key, ev, fl, up, size, weight=None):
    """d (sum upstream . IWE) / d flow [2, H, W] of the float64 oracle's autograd."""
    def make():
        f = torch.from_numpy(fl).clone().requires_grad_(True)
        w = 1.0 if weight is None else torch.from_numpy(weight)
        O.iwe_dense(torch.from_numpy(ev), f, size, weight=w).backward(gradient=torch.from_numpy(up))
        return f.grad.numpy()
    return cached(("ref-up", key, weight is not None), make)


def allowance(counts_px, up_max, dt_bound=1.0):
    """The per-tile absolute allowance of the fixed-point scatter: u / 2 x sqrt(2 sum count^2) with u = 2^-20 x 2 dt_bound max |upstream|,
    the largest unit ``bwd_fx_unit`` can choose at 21 bits; every event is rounded to nearest once per component."""
    u = 2.0 ** -20 * 2.0 * dt_bound * up_max
    return 0.5 * u * float(np.sqrt(2.0 * (counts_px.astype(np.float64) ** 2).sum()))
