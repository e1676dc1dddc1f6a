"""The reference's two time-resolved event representations on the GPU (reference: src/utils/event_utils.py:291-440;
kernels: csrc/event_voxel.hip).

    create_event_voxel                  the DSEC / E2VID voxel grid [C, H, W]: trilinear votes weighted by the signed polarity,
                                        optionally normalised by the mean and std of its non-zero voxels
    generate_discretized_event_volume   the EV-FlowNet / EventGAN volume [T, X, Y]: the two polarities in separate halves, votes
                                        linear in time only
    event_voxel_batch                   the voxel grids of B windows of a recording from its raw sensor columns, in the launches of
                                        one window (``RawEventStore.voxels``)

Every addend of a voxel is the reference's addend bit for bit; they are added by float atomics, so in another order than the
reference's ``put_(accumulate=True)`` and not in the same order from run to run.

Where this differs from the reference: a window whose events all carry one timestamp makes the reference divide by zero and index
with NaN.  The two reference-named calls raise ``ValueError`` for it (and for an empty window); ``event_voxel_batch`` gives such a
window an all-zero grid and a 0 in ``valid``.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip, _staging
from ._hip import check, ptr, stream_ptr


def _shape3(shape, name: str) -> Tuple[int, int, int]:
    try:
        dims = tuple(shape)
    except TypeError:
        dims = ()
    if len(dims) != 3 or any(int(v) != v for v in dims):
        raise ValueError(f"{name} must be three integers, got {shape!r}")
    return tuple(int(v) for v in dims)


def _normalize_(grids: torch.Tensor, lib) -> None:
    """In place, per leading entry of ``grids`` [B, ...]: ``ebos_event_voxel_normalize_f64``."""
    B, n = int(grids.shape[0]), int(grids[0].numel())
    nbytes = int(lib.ebos_event_voxel_normalize_scratch_bytes(B))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=grids.device)
    check(lib.ebos_event_voxel_normalize_f64(B, n, ptr(grids), ptr(scratch), nbytes, stream_ptr(grids.device)),
          "ebos_event_voxel_normalize_f64")


def create_event_voxel(x, y, pol, time, voxel_shape: tuple, normalize: bool = False):
    """Voxel grid with trilinear votes weighted by the polarity (src/utils/event_utils.py:291-366, after DSEC's representations.py).

    Args:
        x ... (n_events, ). x is the width direction.
        y ... (n_events, ).
        pol ... (n_events, ). The polarity, in [-1, +1].
        time ... (n_events, ), sorted.
        voxel_shape (tuple) ... [C, H, W].
        normalize (bool) ... True to map the non-zero voxels to (v - mean) / std (v - mean when std is not > 0).

    Returns:
        voxel_grid ... (voxel_shape), float64: a tensor on the device of ``x``, a numpy array for numpy input.

    torch tensors on any device and numpy arrays are taken; the votes are computed on the GPU.  Unlike the reference, which divides
    by zero and indexes with NaN there, a window with ``time[-1] == time[0]`` (or no event at all) raises ``ValueError``."""
    shapes = [tuple(np.shape(a)) for a in (x, y, pol, time)]
    if any(s != shapes[0] for s in shapes):
        raise ValueError(f"x, y, pol and time must have one shape, got {shapes}")
    if len(shapes[0]) != 1:
        raise ValueError(f"x, y, pol and time must be 1-D, got {len(shapes[0])} dimensions")
    C, H, W = _shape3(voxel_shape, "voxel_shape")
    if C < 1 or H < 1 or W < 1:
        raise ValueError(f"voxel_shape must be positive, got {voxel_shape!r}")
    n = shapes[0][0]
    if n == 0:
        raise ValueError("create_event_voxel: no events, so no time span to divide the bins over")
    kind = _staging.kind_of(x)
    lib = _hip.require_gpu()
    dev = x.device if kind == _staging.GPU else None
    xs, ys, ps, ts = (_staging.to_gpu(a, dev, torch.float64).detach().contiguous() for a in (x, y, pol, time))
    dev = xs.device
    with _hip.on_device(dev):
        grid = torch.empty((C, H, W), dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.ebos_event_voxel_f64(ptr(xs), ptr(ys), ptr(ps), ptr(ts), n, C, H, W, ptr(grid), ptr(status), stream_ptr(dev)),
              "ebos_event_voxel_f64")
        if normalize:
            _normalize_(grid.unsqueeze(0), lib)   # (a grid without a non-zero voxel is left alone, so this may precede the flag)
        if int(status.item()) != 1:
            raise ValueError("create_event_voxel: time[-1] - time[0] is zero or not finite: the events span no time to divide into bins")
    return _staging.back(grid, kind)


def generate_discretized_event_volume(events, vol_size: tuple):
    """Discretised event volume (src/utils/event_utils.py:413-440, after EventGAN's event_utils.py): bins [:T // 2] collect the
    events with p >= 0, bins [T // 2:] those with p < 0, every event votes into the two bins next to its scaled time.

    Args:
        events ... [n_events, 4]. 4 is [x, y, t, p]; x is the height direction.
        vol_size (tuple) ... (T, X, Y) of the returned volume.

    Returns:
        volume ... [T, X, Y] in the events' dtype (float32 stays float32, everything else is float64), in the events' container.

    The reference asserts that every vote falls inside the volume; here a vote outside raises ``ValueError`` (checked on the device,
    one flag read back).  Unlike the reference, which divides by zero there, events that all carry one timestamp raise ``ValueError``."""
    if len(np.shape(events)) != 2 or np.shape(events)[1] != 4:
        raise ValueError(f"events must be [n, 4] = (x, y, t, p), got shape {tuple(np.shape(events))}")
    T, X, Y = _shape3(vol_size, "vol_size")
    if T < 2 or X < 1 or Y < 1:
        raise ValueError(f"vol_size must hold at least two bins (one per polarity) and a positive plane, got {vol_size!r}")
    n = int(np.shape(events)[0])
    if n == 0:
        raise ValueError("generate_discretized_event_volume: no events, so no time span to divide the bins over")
    kind = _staging.kind_of(events)
    lib = _hip.require_gpu()
    ev = _staging.to_gpu(events, events.device if kind == _staging.GPU else None).detach().contiguous()
    dev = ev.device
    with _hip.on_device(dev):
        volume = torch.empty((T, X, Y), dtype=ev.dtype, device=dev)
        status = torch.empty(4, dtype=torch.int64, device=dev)
        fn = getattr(lib, "ebos_event_volume_" + _hip.suffix(ev.dtype))
        check(fn(ptr(ev), n, T, X, Y, ptr(volume), ptr(status), stream_ptr(dev)), "ebos_event_volume")
        flags = int(status[0].item())
    if flags & _hip.EVENT_VOLUME_DEGENERATE_SPAN:
        raise ValueError("generate_discretized_event_volume: all events carry one timestamp (or none that is a number): no span to scale")
    if flags & _hip.EVENT_VOLUME_OUT_OF_BOUNDS:
        raise ValueError(f"generate_discretized_event_volume: events vote outside the volume: x must lie in [0, {X}), y in [0, {Y}) "
                         f"and the scaled time in [0, {T // 2})")
    return _staging.back(volume, kind)


def _roi4(roi, image_shape) -> Optional[Tuple[int, int, int, int]]:
    if roi is None:
        return None
    r = tuple(roi[k] for k in ("xmin", "xmax", "ymin", "ymax")) if isinstance(roi, dict) else tuple(roi)
    if len(r) != 4 or any(int(v) != v for v in r):
        raise ValueError(f"roi must be four integers (xmin, xmax, ymin, ymax), got {roi!r}")
    xmin, xmax, ymin, ymax = (int(v) for v in r)
    H, W = image_shape
    if not (0 <= xmin < xmax <= H and 0 <= ymin < ymax <= W):
        raise ValueError(f"roi rows [{xmin}, {xmax}) x columns [{ymin}, {ymax}) must be non-empty and inside the {H} x {W} sensor")
    return xmin, xmax, ymin, ymax


def event_voxel_batch(columns: Sequence[torch.Tensor], ranges, n_bins: int, image_shape, roi=None, signed: bool = True,
                      normalize: bool = False, ticks_per_second: float = 1e6) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ebos_event_voxel_raw_batch``: the voxel grids of B windows of a recording, from its raw columns, in the launches of one.

    Args:
        columns ... (col int16, row int16, t int32 | int64 ticks, pol uint8 | bool) device columns, as ``RawEventStore.load_raw``
            returns; sorted by time.
        ranges ... B pairs (begin, end) into the columns; they may overlap, may be empty and may come in any order.
        n_bins ... C, the time bins of a grid.
        image_shape ... (H, W) of the sensor.
        roi ... (xmin, xmax = rows, ymin, ymax = columns; tuple or dict) or None.  With it a grid is the crop, [C, xmax - xmin, ymax -
            ymin], and the events outside are dropped before the window's time bounds are taken: ``crop_event`` first.
        signed ... map the polarity {0, 1} to {-1, +1}; False votes with the polarity itself (p = 0 events then vote nothing).
        normalize ... normalise every window's grid on its own, as ``create_event_voxel(..., normalize=True)``.

    Returns:
        grids ... float64 [B, C, H, W] on the columns' device: grid b is ``create_event_voxel(col, row, pol, t / ticks_per_second)``
            of the window's (kept) events, x = column, y = row, so a plane of the grid is an image.
        valid ... int32 [B]: 0 for a window with fewer than two (kept) events or whose first and last share a timestamp; its grid is
            all zero."""
    col, row, t, pol = columns
    for name, c in (("col", col), ("row", row)):
        if not isinstance(c, torch.Tensor) or c.dtype != torch.int16:
            raise ValueError(f"{name} must be an int16 tensor of sensor pixels, got {getattr(c, 'dtype', type(c).__name__)}")
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"t must hold int32 or int64 ticks, got {getattr(t, 'dtype', type(t).__name__)}")
    if isinstance(pol, torch.Tensor) and pol.dtype == torch.bool:
        pol = pol.view(torch.uint8)
    if not isinstance(pol, torch.Tensor) or pol.dtype != torch.uint8:
        raise ValueError(f"pol must be uint8 or bool, got {getattr(pol, 'dtype', type(pol).__name__)}")
    n = int(t.shape[0]) if t.dim() == 1 else -1
    if any(c.dim() != 1 or int(c.shape[0]) != n for c in (col, row, t, pol)):
        raise ValueError("the raw columns must be 1-D and of equal length")
    C = int(n_bins)
    if C != n_bins or C < 1:
        raise ValueError(f"n_bins must be a positive integer, got {n_bins!r}")
    try:
        pairs = [(int(a), int(b)) for a, b in ranges]
    except (TypeError, ValueError) as e:
        raise ValueError(f"ranges must be pairs (begin, end), got {ranges!r}") from e
    if not pairs:
        raise ValueError("ranges holds no window")
    if len(pairs) > 65535:
        raise ValueError(f"{len(pairs)} windows: at most 65535 per call")
    for a, b in pairs:
        if not 0 <= a <= n or not 0 <= b <= n:
            raise ValueError(f"range ({a}, {b}) leaves the {n} events of the columns")
    pairs = [(a, max(a, b)) for a, b in pairs]
    if len(tuple(image_shape)) != 2 or any(int(v) != v or v < 1 for v in image_shape):
        raise ValueError(f"image_shape must be two positive integers (H, W), got {image_shape!r}")
    Hs, Ws = (int(v) for v in image_shape)
    roi = _roi4(roi, (Hs, Ws))
    if not float(ticks_per_second) > 0.0:
        raise ValueError(f"ticks_per_second must be positive, got {ticks_per_second!r}")
    H, W = (roi[1] - roi[0], roi[3] - roi[2]) if roi else (Hs, Ws)
    if not t.is_cuda:
        raise ValueError("the raw columns must be on the GPU (RawEventStore.load_raw)")
    lib = _hip.require_gpu()
    dev = t.device
    col, row, t, pol = (c.contiguous() for c in (col, row, t, pol))
    B = len(pairs)
    with _hip.on_device(dev):
        rng = torch.tensor(pairs, dtype=torch.int64).to(dev, non_blocking=True)
        grids = torch.empty((B, C, H, W), dtype=torch.float64, device=dev)
        valid = torch.empty(B, dtype=torch.int32, device=dev)
        bounds = torch.empty((B, 2), dtype=torch.int64, device=dev)
        check(lib.ebos_event_voxel_raw_batch(ptr(col), ptr(row), ptr(t), int(t.dtype == torch.int64), ptr(pol), n, float(ticks_per_second),
                                             ptr(rng), B, max(b - a for a, b in pairs), C, H, W, int(roi is not None),
                                             *(roi or (0, 0, 0, 0)), int(bool(signed)), ptr(grids), ptr(valid), ptr(bounds),
                                             stream_ptr(dev)), "ebos_event_voxel_raw_batch")
        if normalize:
            _normalize_(grids, lib)
    return grids, valid
