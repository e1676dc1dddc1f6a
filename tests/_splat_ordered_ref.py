"""numpy restatement of the ordered route of the event -> image vote (csrc/splat_ordered.hip, documented in include/ebos_hip.h), for
tests/test_splat_ordered_ref.py (CPU: pinned against the float64 oracle) and tests/test_gpu_splat_ordered.py (the kernels equal it
bit for bit).  Everything is evaluated in the events' dtype, every operation rounded on its own.

The index.  Event ``i = row * n + e`` has the top-left tap ``(R, C) = floor(x + eps) + pad`` (``footprint`` of csrc/common.h).  It is
dropped when a coordinate is NaN, +-Inf or beyond 2^30, or when (R, C) lies outside ``[-1, h - 1] x [-1, w - 1]`` (h, w: the padded
image).  ``key = ((row * planes + plane) * (h + 1) + R + 1) * (w + 1) + C + 1``; ``indices[offsets[k]:offsets[k + 1]]`` are the events
of key k, ascending; the dropped events stand behind ``offsets[keys]``, ascending.

The summation order.  The addend list of pixel (row, plane, r, c): the events of the cells (r - 1, c - 1), (r - 1, c), (r, c - 1), (r, c)
in this order, each cell in ascending event index; the addend is the event's tap on (r, c): ``fr fc wv``, ``fr (1 - fc) wv``,
``(1 - fr) fc wv``, ``(1 - fr)(1 - fc) wv`` as ``(x * y) * wv``; count mode adds 1.
  * at most ``long_list_threshold()`` addends: ``s = +0; s = s + addend`` in list order;
  * more: ``p[l] = +0; p[l] = p[l] + addend[j]`` for ``j = l, l + 64, ...``; then for off = 32, 16, 8, 4, 2, 1:
    ``p[l] = p[l] + p[l + off]`` for ``l < off``; ``s = p[0]``.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "event_based_bos_amd", "csrc", "splat_ordered.hip")
BILINEAR, COUNT, POLARITY = 0, 1, 2
WAVE = 64


def long_list_threshold(source=SOURCE):
    """``kSplatLongList`` as the kernel source states it (never a constant of the tests)."""
    with open(source) as f:
        m = re.search(r"constexpr\s+int\s+kSplatLongList\s*=\s*(\d+)\s*;", f.read())
    if m is None:
        raise RuntimeError("kSplatLongList not found in " + source)
    return int(m.group(1))


def footprints(ev, pad, eps):
    """(R, C int64 [b, n] in padded coordinates, fr, fc in the dtype of ``ev``, finite bool [b, n]) -- ``footprint<T>()``."""
    dt = ev.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        base = np.floor(ev[..., :2] + dt(eps))
        frac = ev[..., :2] - base
        lim = dt(2 ** 30)
        finite = ((base > -lim) & (base < lim)).all(axis=-1)
    whole = np.where(finite[..., None], base, 0).astype(np.int64)
    R = np.where(finite, whole[..., 0] + pad[0], -4)
    C = np.where(finite, whole[..., 1] + pad[1], -4)
    assert frac.dtype == ev.dtype
    return R, C, frac[..., 0], frac[..., 1], finite


def _keys(ev, size, pad, eps, polarity):
    h, w = size
    b, n = ev.shape[:2]
    R, C, fr, fc, finite = footprints(ev, pad, eps)
    keep = finite & (R >= -1) & (R <= h - 1) & (C >= -1) & (C <= w - 1)
    planes = 2 if polarity else 1
    img = np.arange(b, dtype=np.int64)[:, None] * planes + (np.where(ev[..., 3] > 0, 0, 1) if polarity else 0)
    key = (img * (h + 1) + R + 1) * (w + 1) + C + 1
    return key, keep, img, (R, C, fr, fc), b * planes * (h + 1) * (w + 1)


def build_index(ev, size, pad=(0, 0), eps=1e-6, polarity=False):
    """-> (offsets int32 [keys + 1], indices int32 [b * n]) of events [b, n, 4]; ``size`` is the padded (h, w)."""
    key, keep, _, _, n_keys = _keys(ev, size, pad, eps, polarity)
    key, keep = key.reshape(-1), keep.reshape(-1)
    kept = np.flatnonzero(keep)
    order = kept[np.argsort(key[kept], kind="stable")]
    offsets = np.searchsorted(key[order], np.arange(n_keys + 1), side="left")
    return offsets.astype(np.int32), np.concatenate([order, np.flatnonzero(~keep)]).astype(np.int32)


def lists(ev, size, pad=(0, 0), eps=1e-6, polarity=False):
    """The addend lists of every pixel, which do not depend on the weights: (event, q, start) -- addend j of the concatenated lists
    is tap q of event ``event[j]`` (flat index), pixel p owns ``start[p]:start[p + 1]``.  q = 0 .. 3: the event's cell is (r - 1, c - 1),
    (r - 1, c), (r, c - 1), (r, c) of the pixel (r, c) it adds to."""
    h, w = size
    b, n = ev.shape[:2]
    _, keep, img, (R, C, _, _), _ = _keys(ev, size, pad, eps, polarity)
    pix, qs, idx = [], [], []
    event = np.arange(b * n, dtype=np.int64).reshape(b, n)
    for q in range(4):
        r, c = R + (1 if q < 2 else 0), C + (1 if q % 2 == 0 else 0)
        ok = keep & (r >= 0) & (r < h) & (c >= 0) & (c < w)
        pix.append(((img * h + r) * w + c)[ok])
        qs.append(np.full(int(ok.sum()), q, dtype=np.int64))
        idx.append(event[ok])
    pix, qs, idx = (np.concatenate(v) for v in (pix, qs, idx))
    order = np.argsort((pix * 4 + qs) * max(b * n, 1) + idx)    # by pixel, then cell, then event index: the list order (keys are distinct)
    n_pix = b * (2 if polarity else 1) * h * w
    return idx[order], qs[order], np.searchsorted(pix[order], np.arange(n_pix + 1), side="left")


def vote(ev, size, pad=(0, 0), eps=1e-6, weight=1.0, mode=BILINEAR, threshold=None, plan=None):
    """-> image [b, h, w] ([b, 2, h, w] for POLARITY) in the dtype of ``ev`` [b, n, 4]; ``weight`` a number or [b, n].  ``plan``:
    ``lists(ev, size, pad, eps, mode == POLARITY)`` where the caller has them already."""
    threshold = long_list_threshold() if threshold is None else threshold
    dt = ev.dtype.type
    h, w = size
    b, n = ev.shape[:2]
    polarity = mode == POLARITY
    event, qs, start = lists(ev, size, pad, eps, polarity) if plan is None else plan
    if mode == COUNT:
        val = np.ones(len(event), dtype=ev.dtype)
    else:
        _, _, fr, fc, _ = footprints(ev, pad, eps)
        wv = np.asarray(weight, dtype=ev.dtype).reshape(b, n) if isinstance(weight, np.ndarray) else np.full((b, n), dt(weight), dtype=ev.dtype)
        one = dt(1)
        a, bb = one - fr, one - fc
        with np.errstate(invalid="ignore", over="ignore"):       # (dropped events may hold NaN / Inf: their taps are never read)
            taps = np.stack([(fr * fc) * wv, (fr * bb) * wv, (a * fc) * wv, (a * bb) * wv]).reshape(4, b * n)
        val = taps[qs, event]
    assert val.dtype == ev.dtype
    n_pix = len(start) - 1
    length = start[1:] - start[:-1]
    out = np.zeros(n_pix, dtype=ev.dtype)
    short = np.flatnonzero(length <= threshold)
    for j in range(int(length[short].max()) if len(short) else 0):
        sel = short[length[short] > j]
        out[sel] = out[sel] + val[start[sel] + j]
    long_ = np.flatnonzero(length > threshold)
    if len(long_):
        part = np.zeros((len(long_), WAVE), dtype=ev.dtype)
        lanes = np.arange(WAVE)[None, :]
        for j in range(-(-int(length[long_].max()) // WAVE)):
            at = start[long_][:, None] + WAVE * j + lanes
            ok = at < start[long_ + 1][:, None]
            part = part + np.where(ok, val[np.minimum(at, len(val) - 1)], dt(0))   # (x + 0 == x, and no partial sum is -0)
        off = WAVE // 2
        while off:
            part[:, :off] = part[:, :off] + part[:, off:2 * off]
            off //= 2
        out[long_] = part[:, 0]
    assert out.dtype == ev.dtype
    return out.reshape((b, 2, h, w) if polarity else (b, h, w))
