"""Shared cases of tests/test_gpu_voxel_tiles.py (pinned on the CPU by tests/test_voxel_tile_cases.py): what tests/_voxel_loop_cases.py
and tests/_voxel_multiref_cases.py do for a fixed 37 x 70 with plan tile (32, 32), as functions of the image shape, so that every built
(tile_h, tile_w, halo) of the time-aware kernels meets a window in which it has interior tiles, four-window corners and overhang on both
axes, and the pixel-owner backward meets runs of chosen lengths on every tile shape.  The geometry is tests/_hvp_tile_cases.py's, by
import: MAIN = 70 x 135 gives 2 x 3 tiles of (64, 64), 3 x 3 of (32, 64), 3 x 5 of (32, 32) and 5 x 3 of (16, 64).

Windows, all on [0, 1], plan direction "first", every other event with a fractional row (``pool_events``), each event kept MARGIN px
from every integer under the voxel of its case at EVERY reference time of ``ALL`` (first, 0.25, middle, last: one window serves the
single-reference kernels and the K = 1, 3 and 4 cases); offenders are replaced, never dropped, dt == 0 is exempt:

    main      70 x 135, 30 000 events, voxel uniform(-6, 6) per bin: inside every halo >= 8 at every reference time of ``ALL``.
    runs      main with the source pixels of ``RUN_PIXELS`` cleared and refilled to runs of exactly 1 .. 129 events and four hot pixels
              of 300 (``HOT_PIXELS``): two in adjacent columns of one row (two hot lanes of one wave in every tile shape: keys are
              row-major inside a tile), one on (H - 1, W - 1) (the last in-image key of the overhanging corner tile; its wave holds
              lanes outside the image) and one whose key is lane 0 of its wave.  The times of a constructed run are stratified over
              the window (one event per 1 / count of it) and arrive shuffled: its bins come unsorted and, on a hot pixel, fill every
              register slot of the whole-wave walk.
    empty     main without the events of source rows >= 32 and columns >= 64: whole empty tiles of every shape.
    tiny      13 x 21, 600 events: smaller than every tile and every halo.
    batch     [runs, a window of no events, main with another seed and 17 000 events], each under its own voxel.
    spill     main drawn kink-free under uniform(-amp, amp) at first / before / middle / after, amp from ``SPILL_AMP``: at least
              ``SPILL_MIN`` events leave the tile + halo window of their triple and stay inside the image.

Yardsticks, float64 on the CPU through torch autograd, computed once per case (``cached``): tests/_warp_voxel_ref.py (``iwe_voxel``,
``image_variance``), tests/_flow_voxel_grad_ref.py (``voxel_torch``), oracle.ebos_oracle (``upsample_patch_flow``); those of the sibling
case files that do not depend on the image shape are used as they are (``L.ref_variance_grad``, ``M.ref_iwes``,
``M.ref_mean_variance_grad``)."""
import numpy as np
import torch

import _voxel_loop_cases as L
import _voxel_multiref_cases as M
from _hvp_tile_cases import MAIN, MARGIN, N_OF, PATCH, PLAN_TILES, TINY, pool_events, source_pixels  # noqa: F401
from _voxel_loop_cases import G, GR, O, R, cached, dev, rel  # noqa: F401
from _voxel_multiref_cases import FML, FQML

ALL = FQML                                        # every window is kink-free at these reference times ("first" is the plan's own)
BMA = ("before", "middle", "after")               # |dt| reaches 2
DIRECTIONS = {1: ("last",), 3: FML, 4: FQML}
T5 = 5
RUN_T = (64, 65, 129, 255)                        # bins of the runs window beyond the tile sweep's 5
BUILT = ((64, 64, 32), (32, 64, 32), (32, 32, 32), (16, 64, 32), (64, 64, 16), (32, 32, 16), (32, 32, 8), (64, 64, 64), (32, 64, 48))
# source pixel -> its exact run length: both sides of the owner walk's switches at 8 (one chunk) and 64 (the whole-wave path), of
# two chunk boundaries and of two 64-event trips; every tile of the (64, 64) grid holds one of them or a hot pixel
RUN_PIXELS = {(3, 7): 1, (3, 8): 2, (66, 20): 7, (33, 66): 8, (40, 100): 9, (15, 31): 15, (16, 32): 16, (47, 130): 17, (10, 63): 63,
              (10, 64): 64, (31, 31): 65, (50, 20): 127, (64, 64): 128, (69, 100): 129}
HOT_RUN = 300
HOT_PAIR = ((45, 70), (45, 71))
HOT_CORNER = (MAIN[0] - 1, MAIN[1] - 1)
HOT_LANE0 = (22, 64)
HOT_PIXELS = HOT_PAIR + (HOT_CORNER, HOT_LANE0)
CONSTRUCTED = {**RUN_PIXELS, **{p: HOT_RUN for p in HOT_PIXELS}}   # pixel -> run length
WAVE, OWNER_CHUNK, OWNER_HOT, OWNER_SLOTS = 64, 8, 64, 4           # warp_voxel_core.h: kWave, kOwnerChunk, kOwnerHot, kOwnerSlots
BATCH_N2, BATCH_SEED2 = 17_000, 47
# amplitude of the voxel under which at least SPILL_MIN of the 30 000 events leave the triple's tile + halo window inside the image
SPILL_AMP = {(32, 32, 8): 12.0, (32, 32, 16): 40.0, (64, 64, 16): 40.0, (64, 64, 32): 80.0, (32, 64, 32): 80.0, (32, 32, 32): 80.0,
             (16, 64, 32): 80.0, (32, 64, 48): 80.0, (64, 64, 64): 160.0}
SPILL_MIN = 100


def voxel_u(shape, T=T5, amp=6.0, seed=21):
    return L.voxel_u(amp, T, seed, tuple(shape))


def as_list(vx):
    return list(vx) if isinstance(vx, (list, tuple)) else [vx]


def near_kink(ev, vx, directions=ALL, margin=MARGIN):
    """bool [n]: under some direction, and some voxel of ``vx``, the float64-warped event lies within ``margin`` px of an integer."""
    return M._near_kink(ev, as_list(vx), directions, margin)


def off_the_kinks(shape, vx, directions=ALL, seed=41, n=None):
    """``n`` (default N_OF[shape]) events off the kinks of ``vx`` at every direction: the shape-aware twin of
    ``_voxel_multiref_cases.off_the_kinks`` on the candidates of ``_hvp_tile_cases.pool_events``."""
    n = N_OF[tuple(shape)] if n is None else n
    pool = pool_events(shape, n, seed)
    keep = np.ones(len(pool), dtype=bool)
    for _ in range(16):
        ev = np.concatenate([pool[:1], pool[1:-1][keep[1:-1]][:n - 2], pool[-1:]])
        near = near_kink(ev, vx, directions)
        near[0] = near[-1] = False
        if not near.any():
            assert len(ev) == n
            return ev
        keep[np.nonzero(keep[1:-1])[0][:n - 2][near[1:-1]] + 1] = False
    raise AssertionError("no kink-free window found")


def main_window(shape=MAIN, T=T5):
    return cached(("vt-main", tuple(shape), T), lambda: off_the_kinks(shape, voxel_u(shape, T)))


def empty_tiles_window(T=T5):
    """``main_window(MAIN, T)`` without the events of source rows >= 32 and columns >= 64; the first and the last event (t = 0 and 1,
    which set every dt and every bin) stay, moved out of that quarter by whole rows if they lie in it."""
    def make():
        ev = main_window(MAIN, T).copy()
        for i in (0, -1):
            if ev[i, 0] >= 32 and ev[i, 1] >= 64:
                ev[i, 0] -= 32 * (int(ev[i, 0]) // 32)
        r, c = source_pixels(ev)
        out = ev[~((r >= 32) & (c >= 64))]
        assert out[0, 2] == 0.0 and out[-1, 2] == 1.0 and len(out) < len(ev) - 5000
        assert not near_kink(out, voxel_u(MAIN, T))[1:-1].any()
        return out
    return cached(("vt-empty", T), make)


def extras_on(pixel, count, ev, vx, rs):
    """``count`` events on the source pixel, event j at a time inside stratum j of ``count`` equal parts of (0.001, 0.999), each off the
    kinks of ``vx`` at every direction of ``ALL`` (one too close is drawn again inside its stratum)."""
    out = np.zeros((count, 4))
    todo = np.arange(count)
    for _ in range(64):
        m = len(todo)
        out[todo] = np.stack([pixel[0] + rs.uniform(0.02, 0.98, m), pixel[1] + rs.uniform(0.02, 0.98, m),
                              0.001 + 0.998 * (todo + rs.uniform(0.0, 1.0, m)) / count, rs.randint(0, 2, m).astype(np.float64)], axis=1)
        probe = np.concatenate([ev[:1], out[todo], ev[-1:]])                           # (the window stays [0, 1])
        todo = todo[near_kink(probe, vx)[1:-1]]
        if not len(todo):
            return out
    raise AssertionError("no kink-free events found on the pixel")


def runs_window(T=T5, seed=71):
    """``main_window(MAIN, T)`` with the pixels of CONSTRUCTED cleared and refilled to their exact run lengths, the extra events
    shuffled among themselves (not sorted by time), in front of the last event."""
    def make():
        ev, vx, rs = main_window(MAIN, T), voxel_u(MAIN, T), np.random.RandomState(seed)
        r, c = source_pixels(ev)
        chosen = np.zeros(len(ev), dtype=bool)
        for (pr, pc) in CONSTRUCTED:
            chosen |= (r == pr) & (c == pc)
        assert not chosen[0] and not chosen[-1]                                       # the events that set the window stay
        base = ev[~chosen]
        extra = np.concatenate([extras_on(p, k, base, vx, rs) for p, k in CONSTRUCTED.items()])
        extra = extra[rs.permutation(len(extra))]
        out = np.concatenate([base[:-1], extra, base[-1:]])
        assert not near_kink(out, vx)[1:-1].any()
        return out
    return cached(("vt-runs", T, seed), make)


def run_bins(ev, pixel, T):
    """The time bins of the events of one source pixel, in input order."""
    r, c = source_pixels(ev)
    return R.time_bins(ev[:, 2], T)[(r == pixel[0]) & (c == pixel[1])]


def empty_bins_mask(ev, T):
    """bool [T, H, W] over the constructed pixels: the bins a constructed pixel holds no event of."""
    m = np.zeros((T,) + MAIN, dtype=bool)
    for p in CONSTRUCTED:
        m[:, p[0], p[1]] = True
        m[run_bins(ev, p, T), p[0], p[1]] = False
    return m


def key_of(pixel, tile, shape=MAIN):
    """The plan key of a source pixel: tile-major, row-major inside a tile (``owner_bwd_walk`` decodes it back)."""
    th, tw = tile
    tiles_x = -(-shape[1] // tw)
    return ((pixel[0] // th) * tiles_x + pixel[1] // tw) * th * tw + (pixel[0] % th) * tw + pixel[1] % tw


def pixel_of(key, tile, shape=MAIN):
    """(row, column) of a key, or None where the key lies outside the image (the overhang of a tile)."""
    th, tw = tile
    tiles_x = -(-shape[1] // tw)
    t, pit = divmod(key, th * tw)
    r, c = (t // tiles_x) * th + pit // tw, (t % tiles_x) * tw + pit % tw
    return (r, c) if r < shape[0] and c < shape[1] else None


def batch_voxels(T=T5):
    return [voxel_u(MAIN, T, seed=21 + b) for b in range(3)]


def batch_windows(T=T5):
    """[runs, no events, main with another seed and another n (kink-free under voxel 2)]."""
    def make():
        w2 = off_the_kinks(MAIN, batch_voxels(T)[2], seed=BATCH_SEED2, n=BATCH_N2)
        return [runs_window(T), np.zeros((0, 4)), w2]
    return cached(("vt-batch", T), make)


# ---------------------------------------------------------------------------------------------- events beyond the halo
def spill_window(amp, shape=MAIN):
    """Kink-free under uniform(-amp, amp) at the plan's "first" and at before / middle / after."""
    return cached(("vt-spill", amp, tuple(shape)), lambda: off_the_kinks(shape, voxel_u(shape, T5, amp), ("first",) + BMA))


def events_beyond(ev, vx, triple, direction="first"):
    """How many events the tiled forward of this triple hands to its spill path and still votes into the image: the top-left tap
    of the float64 warp outside rows / columns [0, L - 1) of the window of the event's source tile, and inside the image."""
    th, tw, hl = triple
    H, W = vx.shape[-2:]
    warped = R.warp_voxel(torch.from_numpy(ev), torch.from_numpy(vx), direction, True)[0].numpy()
    top = np.floor(warped[:, :2])
    out = np.zeros(len(ev), dtype=bool)
    for axis, t in ((0, th), (1, tw)):
        cell = top[:, axis] - ((ev[:, axis].astype(np.int64) // t) * t - hl)
        out |= (cell < 0) | (cell >= t + 2 * hl - 1)
    inside = (top[:, 0] >= 0) & (top[:, 0] < H) & (top[:, 1] >= 0) & (top[:, 1] < W)
    return int((out & inside).sum())


# ---------------------------------------------------------------------------------------------- float64 yardsticks
def weights_of(n, seed=5):
    """Per-event weights in input order, in [0.5, 1.5]."""
    return cached(("vt-w", n, seed), lambda: np.random.RandomState(seed).uniform(0.5, 1.5, n))


def ref_iwe(key, ev, vx, pad=0, weighted=False, direction="first"):
    """float64 IWE [h, w] of the window under its voxel."""
    def make():
        w = torch.from_numpy(weights_of(len(ev))) if weighted else 1.0
        with torch.no_grad():
            return R.iwe_voxel(torch.from_numpy(ev), torch.from_numpy(vx), direction, True, (pad, pad), w).numpy()
    return cached(("vt-iwe", key, pad, weighted, direction), make)


def ref_iwes(key, ev, vx, directions, pad=0):
    return M.ref_iwes(("vt", key), ev, vx, directions, pad)


def ref_variance_grad(key, ev, vx, omit=False, pad=0):
    return L.ref_variance_grad(("vt", key), ev, vx, omit, pad)


def ref_mean_variance_grad(key, ev, vx, directions, omit=False, pad=0):
    return M.ref_mean_variance_grad(("vt", key), ev, vx, directions, omit, pad)


def column_rel(got, want, pixel):
    """Relative L2 of one source pixel's [T, 2] column of d_voxel against the yardstick's, on its own."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return O.rel_l2(got[:, :, pixel[0], pixel[1]].astype(np.float64), np.asarray(want)[:, :, pixel[0], pixel[1]].astype(np.float64))


# ---------------------------------------------------------------------------------------------- the loop
def theta_start(shape=MAIN, seed=81):
    """[2, gh, gw] float32 in [0.5, 3]: every upwind branch of the voxel is stable (_voxel_loop_cases.theta_start)."""
    gh, gw = O.patch_grid_shape(shape, PATCH, PATCH)
    return cached(("vt-theta", tuple(shape), seed), lambda: np.random.RandomState(seed).uniform(0.5, 3.0, (2, gh, gw)).astype(np.float32))


def ref_voxel(theta, scheme="upwind", shape=MAIN, T=T5):
    dense = O.upsample_patch_flow(theta, shape, PATCH, PATCH)
    return dense, GR.voxel_torch(dense[None], T, scheme, "middle", None)[0]


def ref_loss(theta, ev, directions=("first",), scheme="upwind", shape=MAIN):
    """The float64 objective of the ``time_aware`` block (variance alone) at ``theta``: minus the mean over ``directions``."""
    _, vox = ref_voxel(theta, scheme, shape)
    return -sum(R.image_variance(R.iwe_voxel(torch.from_numpy(ev), vox, d, True)) for d in directions) / len(directions)


def loop_windows(shape=MAIN, scheme="upwind"):
    """[w0, w1]: w0 kink-free at every direction of FML under the float64 voxel of theta_start(), w1 its first, every third
    interior and last event (the time range, and so every kept event's bin and warp, is unchanged)."""
    def make():
        with torch.no_grad():
            _, vox = ref_voxel(torch.from_numpy(theta_start(shape)).double(), scheme, shape)
        w0 = off_the_kinks(shape, vox.numpy(), FML, seed=53)
        return [w0, np.concatenate([w0[:1], w0[1:-1][::3], w0[-1:]])]
    return cached(("vt-loop-ev", tuple(shape), scheme), make)


def ref_value_and_grad(b, directions=("first",), scheme="upwind", shape=MAIN):
    """(loss, d loss / d theta) of window b of ``loop_windows`` at theta_start()."""
    def make():
        th = torch.from_numpy(theta_start(shape)).double().requires_grad_(True)
        loss = ref_loss(th, loop_windows(shape, scheme)[b], directions, scheme, shape)
        loss.backward()
        return loss.item(), th.grad.numpy()
    return cached(("vt-loop-grad", b, tuple(directions), scheme, tuple(shape)), make)
