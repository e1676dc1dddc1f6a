"""Cases of tests/test_gpu_ops.py (pinned on the CPU by tests/test_ops_cases.py): the general kernels behind ``event_based_bos_amd.ops``
-- csrc/warp_kernels.hip, splat_kernels.hip, cost_kernels.hip (``moments`` / ``gradmag`` / ``*_grad``) and image_filters.hip -- at the
smallest shapes at which each of them can still go wrong: past one launch wave (a second, ragged trip of every grid-stride loop),
past ``kCostGrid`` rows and ``kCostBlock`` columns of a cost region, with ``K > 1`` stacks and ``b > 1`` batches, in both dtypes.

The launch limits are READ from the C sources (``limits``): the default ``max_blocks`` of ``stream_grid`` in common.h, the explicit cap
at every call site, ``kCostGrid`` and ``kCostBlock``.  A limit that cannot be found is an error, never a constant of this file, so the
claims below (``claims()``: which kernel meets which case, with how many items) are checked against the kernels as they are:
tests/test_ops_cases.py computes the trips of every claim and fails when a cap has been raised past its case.

Inputs come from ``numpy.random.RandomState`` alone.  Everything is importable without a GPU.

    events       [b, n, 4] (row, column, t, p).  float32 cases keep the coordinates on a 1/64 px grid (exact in float32: the kernel and
                 the float64 oracle floor the same numbers).  ``splat_events``: every 8th event is an EDGE event, each axis
                 independently inside the padded image, in (-pad - 1, -pad) (the first tap of the axis masked), equal to the last
                 padded row / column (the second tap masked) or beyond it (both masked): each of the four taps is masked on its own.
                 The polarity cycles through 1, 0, 1, -1.  ``warp_events``: sources inside the flow field, with an event every
                 ``OOR_EVERY`` whose source pixel lies outside it (``oor_indices``: some in every trip of the loop).
    timestamps   sorted in [1.0, 1.4]; ``mixed_t`` cases draw them from (-0.3, 0.2), unsorted, the minimum planted in the second trip
                 of the 1024-cap loop and the maximum in its third.
    images       [K, h, w]: smooth plus noise, mean about 3, rising towards the last rows and columns (so that rows beyond
                 ``kCostGrid`` and columns beyond ``kCostBlock`` weigh in the moments).
"""
import functools
import os
import re
from dataclasses import dataclass

import numpy as np
import torch

from oracle import ebos_oracle as O

from _kinks import off_the_kinks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "event_based_bos_amd", "csrc")

# kernel -> the source file that launches it.  Grid-stride kernels (their launch takes its grid from stream_grid):
STREAM_KERNELS = {
    "time_range_kernel": "warp_kernels.hip", "warp_dense_kernel": "warp_kernels.hip", "warp_dense_bwd_kernel": "warp_kernels.hip",
    "warp_2dof_kernel": "warp_kernels.hip", "warp_2dof_bwd_kernel": "warp_kernels.hip",
    "splat_kernel": "splat_kernels.hip", "splat_bwd_kernel": "splat_kernels.hip",
    "variance_grad_kernel": "cost_kernels.hip", "gradmag_grad_kernel": "cost_kernels.hip",
    "gauss1d_kernel": "image_filters.hip", "gauss1d_bwd_kernel": "image_filters.hip",
}
EVENT_KERNELS = tuple(k for k, f in STREAM_KERNELS.items() if f in ("warp_kernels.hip", "splat_kernels.hip"))
PIXEL_KERNELS = tuple(k for k in STREAM_KERNELS if k not in EVENT_KERNELS)
REGION_KERNELS = ("moments_kernel", "gradmag_kernel")   # rows step by kCostGrid, columns by kCostBlock


class LimitNotFound(RuntimeError):
    pass


def _read(csrc, name):
    with open(os.path.join(csrc, name)) as f:
        return f.read()


def _int_expr(text, consts):
    """A product of integer literals and known constants (``256 * 8``, ``kCostBlock``)."""
    value = 1
    for factor in text.split("*"):
        factor = factor.strip()
        if re.fullmatch(r"\d+", factor):
            value *= int(factor)
        elif factor in consts:
            value *= consts[factor]
        else:
            raise LimitNotFound(f"cannot evaluate {text!r}")
    return value


def _constexpr(text, name, where):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9* ]+);", text)
    if m is None:
        raise LimitNotFound(f"{name} not found in {where}")
    return _int_expr(m.group(1), {})


def _split_args(text):
    args, depth, cur = [], 0, ""
    for ch in text:
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
            continue
        depth += ch in "(<"
        depth -= ch in ")>"
        cur += ch
    return args + [cur.strip()]


_STREAM_GRID_CALL = re.compile(r"stream_grid\(((?:[^()]|\((?:[^()]|\([^()]*\))*\))*)\)")


def limits(csrc=CSRC):
    """{"default_cap", "kCostGrid", "kCostBlock", kernel: (block, cap) for every kernel of STREAM_KERNELS}, parsed from the sources in
    ``csrc``.  Every launch of a kernel must take its grid from the same stream_grid call."""
    out = {}
    common = _read(csrc, "common.h")
    m = re.search(r"\bint\s+stream_grid\s*\([^)]*\bint\s+max_blocks\s*=\s*([0-9* ]+)\)", common)
    if m is None:
        raise LimitNotFound("the default max_blocks of stream_grid not found in common.h")
    out["default_cap"] = _int_expr(m.group(1), {})
    cost = _read(csrc, "cost_kernels.hip")
    out["kCostGrid"] = _constexpr(cost, "kCostGrid", "cost_kernels.hip")
    out["kCostBlock"] = _constexpr(cost, "kCostBlock", "cost_kernels.hip")
    for kernel in REGION_KERNELS:   # launched on dim3(kCostGrid, K) x dim3(kCostBlock), nothing else
        if re.search(r"\b" + kernel + r"\s*<[^<>]*>\s*<<<\s*dim3\(kCostGrid,\s*K\),\s*dim3\(kCostBlock\)", cost) is None:
            raise LimitNotFound(f"the launch of {kernel} on dim3(kCostGrid, K) x dim3(kCostBlock) not found in cost_kernels.hip")
    consts = {"kCostBlock": out["kCostBlock"]}
    for kernel, name in STREAM_KERNELS.items():
        text = cost if name == "cost_kernels.hip" else _read(csrc, name)
        found = set()
        for launch in re.finditer(r"\b" + kernel + r"\s*(?:<[^<>]*>)?\s*<<<", text):
            end = text.index(">>>", launch.end())
            calls = [c for c in _STREAM_GRID_CALL.finditer(text, 0, end)]
            if not calls or "\n}\n" in text[calls[-1].end():end]:
                raise LimitNotFound(f"no stream_grid call in the function that launches {kernel} ({name})")
            args = _split_args(calls[-1].group(1))
            if len(args) not in (2, 3):
                raise LimitNotFound(f"stream_grid call of {kernel}: {calls[-1].group(0)!r}")
            found.add((_int_expr(args[1], consts), _int_expr(args[2], consts) if len(args) == 3 else out["default_cap"]))
        if len(found) != 1:
            raise LimitNotFound(f"{kernel}: expected one launch geometry in {name}, found {sorted(found)}")
        out[kernel] = found.pop()
    return out


def trips(items, block, cap):
    """(trips of the grid-stride loop, items of the last trip, items per full trip) of a launch of stream_grid(items, block, cap)."""
    grid = max(1, min(-(-items // block), cap))
    wave = grid * block
    n_trips = -(-items // wave)
    return n_trips, items - (n_trips - 1) * wave, wave


# ---------------------------------------------------------------------------------------------------------------- the shapes
N_BIG = 600_037           # above 2 x 1024 x 256 and above 2048 x 256, no multiple of 256: two ragged trips under the 2048 cap, three under 1024
EVENT_IMAGE = (37, 53)    # the image of the event cases (odd, no multiple of anything)
SMALL_N = (0, 1, 255, 256, 257)
COST_IMAGE = (243, 259)   # cropped by omit_boundary it still has more than kCostGrid rows and more than kCostBlock columns
PIXEL_IMAGE = (601, 1801)  # 1 082 401 pixels: just above 4096 x 256, the largest cap of an element-wise pass
DEGENERATE = ((1, 1), (1, 7), (2, 5), (3, 3))
GAUSS_CASES = tuple((axis, boundary, radius) for axis in (0, 1) for boundary in (0, 1) for radius in (1, 6))
EDGE_EVERY, OOR_EVERY = 8, 997
DTYPES = (np.float32, np.float64)

# the project's bars (header of tests/test_gpu_parity.py); warped events are bit-exact
BARS = {np.float64: {"image": 1e-12, "cost": 1e-12, "grad": 1e-10}, np.float32: {"image": 1e-5, "cost": 1e-5, "grad": 1e-3}}


def bar(dtype, what):
    return BARS[np.dtype(dtype).type][what]


def passes(err, dtype, what):
    """float64 bars are inclusive (<=), float32 bars strict (<), as the project states them."""
    b = bar(dtype, what)
    return err <= b if np.dtype(dtype) == np.float64 else err < b


@dataclass(frozen=True)
class EventCase:
    b: int
    n: int
    dtype: type
    pad: int = 0
    mixed_t: bool = False
    seed: int = 11

    @property
    def id(self):
        return f"b{self.b}-n{self.n}-{np.dtype(self.dtype).name}-pad{self.pad}" + ("-mixed" if self.mixed_t else "")


BIG_EVENT_CASES = tuple(EventCase(b, N_BIG, dt, pad) for dt in DTYPES for b in (1, 3) for pad in (0, 2))
MIXED_CASES = tuple(EventCase(3, N_BIG, dt, 0, True) for dt in DTYPES)     # one per dtype
SMALL_EVENT_CASES = tuple(EventCase(3, n, dt, pad) for dt in DTYPES for n in SMALL_N for pad in (0, 2))


def claims():
    """(kernel, case id, items) for the grid-stride kernels and (kernel, case id, region rows, region columns) for the reductions:
    what tests/test_gpu_ops.py relies on to reach the second trip of each loop."""
    out = [(k, f"n_big {N_BIG}", N_BIG) for k in EVENT_KERNELS]
    out += [(k, "pixels %dx%d" % PIXEL_IMAGE, PIXEL_IMAGE[0] * PIXEL_IMAGE[1]) for k in PIXEL_KERNELS]
    for omit in (0, 1):
        out += [(k, "cost %dx%d omit %d" % (COST_IMAGE + (omit,)), COST_IMAGE[0] - 2 * omit, COST_IMAGE[1] - 2 * omit)
                for k in REGION_KERNELS]
    return out


# ---------------------------------------------------------------------------------------------------------------- events
def _grid64(rs, hi, size):
    """Coordinates in [0, hi) on the 1/64 px grid."""
    return rs.randint(0, int(hi) * 64, size) / 64.0


def _timestamps(rs, case, wave1024):
    b, n = case.b, case.n
    if not case.mixed_t:
        return np.sort(rs.uniform(1.0, 1.4, (b, n)), axis=1)
    t = rs.uniform(-0.3, 0.2, (b, n))
    for r in range(b):   # the extremes past the first trip: minimum in the second trip of the 1024-cap loop, maximum in its third
        t[r, wave1024 + 17 + r] = -0.31 - 0.01 * r
        t[r, 2 * wave1024 + 29 + r] = 0.21 + 0.01 * r
    return t


def _wave(kernel):
    block, cap = limits()[kernel]
    return block * cap


_CATS = ("inside", "first_masked", "second_masked", "both_masked")


def edge_categories(n):
    """For the edge events of a window of n events: (indices, row category, column category), categories indexing _CATS; every
    pair but (inside, inside) in turn."""
    idx = np.arange(3, n, EDGE_EVERY)
    pair = 1 + np.arange(len(idx)) % 15
    return idx, pair // 4, pair % 4


def _edge_value(rs, cat, size, pad, count):
    """Coordinates of one axis of ``size`` (un-padded) for categories ``cat``."""
    k = rs.randint(1, 64, count) / 64.0
    inside = _grid64(rs, size - 1, count)
    return np.select([cat == 0, cat == 1, cat == 2], [inside, -pad - k, np.full(count, size + pad - 1.0)], size + pad + k - 1.0 / 64)


@functools.lru_cache(maxsize=4)
def splat_events(case):
    """[b, n, 4] in ``case.dtype``: (already warped) events for the accumulation kernels, coordinates relative to the un-padded image
    of EVENT_IMAGE; every EDGE_EVERY-th is an edge event (``edge_categories``)."""
    rs = np.random.RandomState(case.seed)
    h, w = EVENT_IMAGE
    b, n = case.b, case.n
    ev = np.zeros((b, n, 4))
    ev[..., 0] = _grid64(rs, h - 1, (b, n))
    ev[..., 1] = _grid64(rs, w - 1, (b, n))
    idx, rc, cc = edge_categories(n)
    for r in range(b):
        ev[r, idx, 0] = _edge_value(rs, rc, h, case.pad, len(idx))
        ev[r, idx, 1] = _edge_value(rs, cc, w, case.pad, len(idx))
    if n:
        ev[..., 2] = _timestamps(rs, case, _wave("time_range_kernel"))
    ev[..., 3] = np.array([1.0, 0.0, 1.0, -1.0])[np.arange(n) % 4]
    return np.ascontiguousarray(ev.astype(case.dtype))


def stated_masked_taps(case):
    """The number of masked taps per batch row, from the construction alone: an axis has 2, 1, 1, 0 valid taps by category."""
    _, rc, cc = edge_categories(case.n)
    valid = np.array([2, 1, 1, 0])
    return int((4 - valid[rc] * valid[cc]).sum())


def stated_nonpositive_polarity(case):
    return case.n // 4 + (case.n + 2) // 4     # i % 4 == 1 and i % 4 == 3


def counted_masked_taps(ev, pad):
    """[b, n] masked taps per event by the oracle's own tap masks."""
    return (~tap_masks(ev, pad)).sum(axis=1)


def tap_masks(ev, pad):
    """bool [b, 4, n]: the oracle's validity masks of the taps (r, c), (r + 1, c), (r, c + 1), (r + 1, c + 1)."""
    h, w = EVENT_IMAGE
    ev = np.asarray(ev, dtype=np.float64)
    _, _, mask = O._taps_numpy(ev[..., :2], h + 2 * pad, w + 2 * pad, pad, pad, O.EPS_TORCH)
    return mask.reshape(ev.shape[0], 4, ev.shape[1])


def oor_indices(n):
    return np.arange(5, n, OOR_EVERY)


def oor_per_trip(n, kernel="warp_dense_kernel"):
    """How many out-of-range events lie in each trip of the kernel's loop."""
    block, cap = limits()[kernel]
    n_trips, _, wave = trips(n, block, cap)
    idx = oor_indices(n)
    return [int(((idx >= k * wave) & (idx < (k + 1) * wave)).sum()) for k in range(n_trips)]


@functools.lru_cache(maxsize=4)
def warp_events(case):
    """[b, n, 4] in ``case.dtype``: source events inside the flow field of EVENT_IMAGE, the events of ``oor_indices`` outside it
    (alternately a row >= h and a negative flattened index)."""
    rs = np.random.RandomState(case.seed + 100)
    h, w = EVENT_IMAGE
    b, n = case.b, case.n
    ev = np.zeros((b, n, 4))
    ev[..., 0] = _grid64(rs, h, (b, n))
    ev[..., 1] = _grid64(rs, w, (b, n))
    idx = oor_indices(n)
    far = np.where(np.arange(len(idx)) % 2 == 0, h + rs.randint(0, 9, len(idx)) + 0.25, -2.0 - rs.randint(0, 9, len(idx)) - 0.5)
    ev[:, idx, 0] = far
    if n:
        ev[..., 2] = _timestamps(rs, case, _wave("time_range_kernel"))
    ev[..., 3] = rs.randint(0, 2, (b, n))
    return np.ascontiguousarray(ev.astype(case.dtype))


def source_out_of_range(ev):
    """bool [b, n]: the flattened source index of src/warp.py:334 (truncation toward zero) lies outside the flow field."""
    h, w = EVENT_IMAGE
    lin = np.trunc(ev[..., 0]).astype(np.int64) * w + np.trunc(ev[..., 1]).astype(np.int64)
    return (lin < 0) | (lin >= h * w)


def flow_of(case, amp=3.0):
    """[b, 2, h, w] in ``case.dtype``."""
    rs = np.random.RandomState(case.seed + 200)
    return rs.uniform(-amp, amp, (case.b, 2) + EVENT_IMAGE).astype(case.dtype)


def weights_of(case):
    return np.random.RandomState(case.seed + 300).uniform(0.5, 1.5, (case.b, case.n)).astype(case.dtype)


def upstream_events(case, seed=400):
    """[b, n, 4] upstream gradient of warped events, mean 0.5 (a float32 sum over the events does not cancel)."""
    return (0.5 + np.random.RandomState(case.seed + seed).normal(size=(case.b, case.n, 4))).astype(case.dtype)


def upstream_image(case, seed=500):
    h, w = EVENT_IMAGE
    return np.random.RandomState(case.seed + seed).normal(size=(case.b, h + 2 * case.pad, w + 2 * case.pad)).astype(case.dtype)


DUPLICATES = 4096   # events planted on ONE source pixel in every batch row: the atomics of warp_dense_bwd meet on one address


def with_duplicates(ev):
    """``warp_events`` with DUPLICATES in-range events (spread over the window) moved onto source pixel (17, 23)."""
    ev = ev.copy()
    n = ev.shape[1]
    idx = np.setdiff1d(np.arange(1, n, max(1, n // DUPLICATES)), oor_indices(n))[:DUPLICATES]
    ev[:, idx, 0] = 17.25
    ev[:, idx, 1] = 23.5
    return ev


# ---------------------------------------------------------------------------------------------------------------- oracle (float64, CPU)
def T64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def ref_warp_dense(ev, flow, direction, normalize_t):
    """The oracle's torch branch in the dtype of ``ev`` ([b, n, 4]); the reference raises for a source outside the flow field, the
    kernels count such events and leave their coordinates as they are (t still becomes dt): restated here on top of the oracle."""
    bad = source_out_of_range(ev)
    safe = ev.copy()
    safe[bad, 0] = 0.0
    safe[bad, 1] = 0.0
    out = O.warp_dense_torch(torch.from_numpy(safe), torch.from_numpy(flow), direction, normalize_t).numpy().reshape(ev.shape)
    out[bad, 0] = ev[bad, 0]
    out[bad, 1] = ev[bad, 1]
    return out, bad


def padded(pad):
    return (EVENT_IMAGE[0] + 2 * pad, EVENT_IMAGE[1] + 2 * pad)


def ref_splat(ev, pad, weight=1.0):
    """float64 bilinear vote [b, H, W] of the values of ``ev`` (upcast), eps of the tensor branch."""
    w = T64(weight) if isinstance(weight, np.ndarray) else weight
    return O.bilinear_vote_torch(T64(ev), padded(pad), (pad, pad), w).reshape((ev.shape[0],) + padded(pad)).numpy()


def ref_splat_f32_in_order(ev, pad, weight):
    """The same sum in float32 on the CPU, ``np.add.at`` in input order: what float32 accumulation alone costs.  Per-event weights
    [b, n]: with unit weight the taps of events on the 1/64 px grid are multiples of 1 / 4096 and a float32 sum of them is exact."""
    h, w = padded(pad)
    e = ev.astype(np.float32)
    base = np.floor(e[..., :2] + np.float32(O.EPS_TORCH))
    frac = (e[..., :2] - base).astype(np.float32)
    row, col = base[..., 0].astype(np.int64) + pad, base[..., 1].astype(np.int64) + pad
    one = np.float32(1)
    wt = np.asarray(weight, dtype=np.float32)
    out = np.zeros((e.shape[0], h * w), dtype=np.float32)
    for b in range(e.shape[0]):
        for dr, dc, val in ((0, 0, (one - frac[b, :, 0]) * (one - frac[b, :, 1])), (1, 0, frac[b, :, 0] * (one - frac[b, :, 1])),
                            (0, 1, (one - frac[b, :, 0]) * frac[b, :, 1]), (1, 1, frac[b, :, 0] * frac[b, :, 1])):
            r, c = row[b] + dr, col[b] + dc
            ok = (r >= 0) & (r < h) & (c >= 0) & (c < w)
            np.add.at(out[b], (r * w + c)[ok], (val * wt[b])[ok].astype(np.float32))
    return out.reshape(e.shape[0], h, w)


def ref_count(ev, pad):
    return O.count_events_numpy(np.asarray(ev, dtype=np.float64), padded(pad), (pad, pad), eps=O.EPS_TORCH).reshape((ev.shape[0],) + padded(pad))


def ref_polarity(ev, pad, weight=1.0):
    """[b, 2, H, W], row by row: the votes of the events of polarity > 0 and of the others (src/event_image_converter.py:355-363)."""
    ev = np.asarray(ev, dtype=np.float64)
    out = []
    for r in range(ev.shape[0]):
        pos = ev[r, :, 3] > 0
        out.append(np.stack([ref_splat(ev[r:r + 1, m], pad, weight[r:r + 1, m] if isinstance(weight, np.ndarray) else weight)[0]
                             for m in (pos, ~pos)]))
    return np.stack(out)


def ref_splat_backward(ev, pad, weight, upstream):
    """(d events [b, n, 4], d weight [b, n]) of <bilinear vote, upstream>, float64 autograd of the oracle."""
    e = T64(ev).requires_grad_(True)
    w = T64(weight).requires_grad_(True)
    img = O.bilinear_vote_torch(e, padded(pad), (pad, pad), w).reshape((ev.shape[0],) + padded(pad))
    (img * T64(upstream)).sum().backward()
    return e.grad.numpy(), w.grad.numpy()


def ref_warp_dense_backward(ev, flow, direction, normalize_t, upstream):
    """d flow [b, 2, h, w] of <warp_dense, upstream>; out-of-range events contribute nothing."""
    bad = source_out_of_range(ev)
    safe = np.asarray(ev, dtype=np.float64).copy()
    safe[bad, 0] = 0.0
    safe[bad, 1] = 0.0
    f = T64(flow).requires_grad_(True)
    out = O.warp_dense_torch(torch.from_numpy(safe), f, direction, normalize_t).reshape(ev.shape)
    up = np.asarray(upstream, dtype=np.float64).copy()
    up[bad] = 0.0
    (out * torch.from_numpy(up)).sum().backward()
    return f.grad.numpy()


def ref_warp_2dof_backward(ev, theta, direction, normalize_t, upstream):
    th = T64(theta).requires_grad_(True)
    out = O.warp_2dof(T64(ev), th, direction, normalize_t)
    (out * T64(upstream)).sum().backward()
    return th.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------- images
@functools.lru_cache(maxsize=8)
def images(K, shape, dtype, seed=31):
    """[K, h, w] in ``dtype``: smooth plus noise, mean about 3, rising towards the last rows and columns; image k has its own phase."""
    h, w = shape
    rs = np.random.RandomState(seed)
    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    out = np.stack([3.0 + 1.5 * np.sin(r / 7.0 + k) * np.cos(c / 11.0 - k) + 4.0 * np.exp((r - h + 1) / 2.0) + 4.0 * np.exp((c - w + 1) / 2.0)
                    + 0.3 * rs.normal(size=(h, w)) for k in range(K)])
    return out.astype(dtype)


def upstream_costs(K, dtype):
    """A different upstream gradient per image of a stack."""
    return np.array([0.7, -1.3, 2.1])[:K].astype(dtype)


COSTS = {"var": O.image_variance, "gm": O.gradient_magnitude}


def ref_cost(name, imgs, omit, upstream=None):
    """(values [K], d <values, upstream> / d images [K, h, w]) by the oracle in float64 on the upcast values."""
    x = T64(imgs).requires_grad_(True)
    vals = torch.stack([COSTS[name](x[k], omit, "maximize") for k in range(x.shape[0])])
    up = torch.ones(x.shape[0], dtype=torch.float64) if upstream is None else T64(upstream)
    (vals * up).sum().backward()
    return vals.detach().numpy(), x.grad.numpy()


def gauss_taps(radius, seed=5):
    """2 radius + 1 positive taps, NOT symmetric: a pass that read them mirrored would show."""
    return np.random.RandomState(seed + radius).uniform(0.1, 1.0, 2 * radius + 1)


def gauss_operator(L, taps, boundary):
    """A[i, j] = d out[i] / d in[j] of one blur pass, from the library the reference calls: scipy correlate1d 'reflect' (boundary 0)
    or torch reflect pad + conv1d (boundary 1), as test_blur_pass_adjoint builds it."""
    radius = (len(taps) - 1) // 2
    eye = np.eye(L)
    if boundary == 0:
        from scipy.ndimage import correlate1d

        return correlate1d(eye, taps, axis=0, mode="reflect")
    pad = torch.nn.functional.pad(torch.from_numpy(eye.T)[None], (radius, radius), mode="reflect")[0]
    return torch.nn.functional.conv1d(pad[:, None], torch.from_numpy(taps)[None, None])[:, 0].numpy().T


def apply_along(A, x, axis):
    return np.moveaxis(np.tensordot(A, np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0), axes=1), 0, axis)


# ---------------------------------------------------------------------------------------------------------------- the chain
CHAIN_DIRECTION, CHAIN_OMIT = "first", True


@functools.lru_cache(maxsize=2)
def chain_inputs(dtype, b=3, n=N_BIG, seed=61):
    """(events [b, n, 4], flow [b, 2, h, w]) in ``dtype`` for warp -> splat -> variance -> backward: no event within 5e-4 px of a
    kink of the vote under the float64 warp (tests/_kinks.py, as the fused fuzz does; the first and the last event of a row, which
    set its time range, stay)."""
    rs = np.random.RandomState(seed)
    h, w = EVENT_IMAGE
    flow = rs.uniform(-3.0, 3.0, (b, 2, h, w)).astype(dtype)
    rows = []
    for r in range(b):
        m = n + n // 50
        ev = np.stack([_grid64(rs, h, m), _grid64(rs, w, m), np.sort(rs.uniform(1.0, 1.4, m)), rs.randint(0, 2, m).astype(np.float64)], 1)
        ev = ev.astype(dtype).astype(np.float64)      # the values the kernel sees, upcast
        ev = off_the_kinks(ev, flow[r].astype(np.float64), CHAIN_DIRECTION, 3.0)
        assert len(ev) >= n
        rows.append(np.concatenate([ev[:n - 1], ev[-1:]]))   # the time range of the filtered row is kept
    return np.ascontiguousarray(np.stack(rows).astype(dtype)), flow


def ref_chain(ev, flow, pad, upstream):
    """(warped [b, n, 4], iwe [b, H, W], variance [b], d <variance, upstream> / d flow) in float64."""
    f = T64(flow).requires_grad_(True)
    warped = O.warp_dense_torch(T64(ev), f, CHAIN_DIRECTION, True).reshape(ev.shape)
    iwe = O.bilinear_vote_torch(warped, padded(pad), (pad, pad)).reshape((ev.shape[0],) + padded(pad))
    var = torch.stack([O.image_variance(iwe[k], CHAIN_OMIT, "maximize") for k in range(iwe.shape[0])])
    (var * T64(upstream)).sum().backward()
    return warped.detach().numpy(), iwe.detach().numpy(), var.detach().numpy(), f.grad.numpy()


def rel(a, b):
    return O.rel_l2(a, b)
