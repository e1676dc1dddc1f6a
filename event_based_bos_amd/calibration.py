"""Lens calibration on the GPU: from a camera matrix ``K`` and distortion coefficients ``D`` to rectified sub-pixel events and
rectified frames (reference: ``utils.undistort_events``, src/utils/event_utils.py:242-266; the loaders' ``load_calib() -> {"K", "D"}``
and ``undistort(event_batch)``, src/data_loader/ccs.py:427-451; ``SolverBase.undistort_image``, src/solver/base.py:363-378).

The reference's surface for calibration is small and half-finished: its loaders return no calibration and refuse ``undistort``.
This module supplies the model those names need and the kernels (csrc/rectify.hip) that put a calibrated recording on the
fractional-coordinate ("undistorted events") path of ``EventPlan.build`` and the resident loops.

Conventions, used everywhere:

* ``K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]``: ``cx`` and ``fx`` belong to the COLUMN axis (sensor x), ``cy`` and ``fy`` to the ROW
  axis.
* ``D`` is in OpenCV's order with 4, 5 or 8 coefficients ``(k1, k2, p1, p2[, k3[, k4, k5, k6]])``; any other length raises
  ``ValueError`` (the 12- and 14-coefficient thin-prism / tilted models and the fisheye model are out of scope).
* Events stay ``(x = row, y = col, t, p)``, as everywhere in this package; points are ``(row, col)`` pairs.

The forward model maps an ideal normalised ``(x, y)`` to a sensor pixel ``(u, v)`` (every operation rounded on its own)::

    r2 = x*x + y*y
    rad = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
    a = (2*x)*y;  dx = p1*a + p2*(r2 + 2*(x*x));  dy = p1*(r2 + 2*(y*y)) + p2*a
    u = fx*(x*rad + dx) + cx;  v = fy*(y*rad + dy) + cy

The inverse is the usual fixed-point iteration with a FIXED count (``iterations``, default 20), so no bit depends on a convergence
test: from ``x0 = (u - cx)/fx``, ``y0 = (v - cy)/fy`` repeat ``x = (x0 - dx(x, y))/rad(x, y)``, ``y = (y0 - dy(x, y))/rad(x, y)``
starting at ``(x0, y0)``; the rectified pixel is ``(fx'*x + cx', fy'*y + cy')`` under ``new_K``, which defaults to ``K``.

Out of scope: ``cv2.getOptimalNewCameraMatrix`` and with it the reference's ``SolverBase.undistort_image`` as written.  OpenCV is
absent where this package is developed and its rectangle search cannot be pinned by a test; ``new_K`` is the caller's.  The image
path (``frame_warp.undistort_image``) is checked against tests/_rectify_ref.py and the forward model, not against ``cv2.undistort``.

There is no CPU computation apart from ``distort_points``: without a GPU the calls raise ``HipUnavailableError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import check, stream_ptr
from ._staging import default_device

MAX_EVENTS = 2147000000   # EBOS_RECTIFY_MAX_EVENTS: the compaction's offsets are int32


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _matrix(K, name: str) -> np.ndarray:
    try:
        k = np.array(K, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise ValueError(f"{name} must be a 3 x 3 matrix of numbers: {err}") from None
    if k.shape != (3, 3) or not np.isfinite(k).all():
        raise ValueError(f"{name} must be a finite 3 x 3 matrix, got shape {k.shape}")
    if k[0, 1] != 0 or k[1, 0] != 0 or k[2, 0] != 0 or k[2, 1] != 0 or k[2, 2] != 1:
        raise ValueError(f"{name} must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew), got {k.tolist()}")
    if k[0, 0] == 0 or k[1, 1] == 0:
        raise ValueError(f"{name} is not invertible: fx = {k[0, 0]}, fy = {k[1, 1]}")
    return k


class CameraCalibration(object):
    """A pinhole camera with OpenCV's rational-polynomial lens model.

    Args:
        K ... 3 x 3 camera matrix (see the module docstring for the axes).
        D ... 4, 5 or 8 distortion coefficients in OpenCV's order.
        sensor_size ... (height, width) of the sensor the calibration belongs to.
        new_K ... camera matrix of the rectified image; None = ``K``.
        iterations ... fixed number of steps of the inverse iteration (>= 1).
    """
    def __init__(self, K, D, sensor_size: Tuple[int, int], new_K=None, iterations: int = 20):
        self.K = _matrix(K, "K")
        try:
            d = np.array(D, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError) as err:
            raise ValueError(f"D must be a sequence of numbers: {err}") from None
        if d.size not in (4, 5, 8):
            raise ValueError(f"D must hold 4, 5 or 8 coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got {d.size}")
        if not np.isfinite(d).all():
            raise ValueError("D has entries that are not finite")
        self.D = d
        self.new_K = self.K.copy() if new_K is None else _matrix(new_K, "new_K")
        try:
            H, W = sensor_size
            ok = int(H) == H and int(W) == W and 0 < H <= 32767 and 0 < W <= 32767
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"sensor_size must be (height, width) with 1 .. 32767 pixels a side, got {sensor_size!r}")
        self.sensor_size = (int(H), int(W))
        try:
            ok = int(iterations) == iterations and 1 <= iterations <= 1000
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"iterations must be an integer in 1 .. 1000, got {iterations!r}")
        self.iterations = int(iterations)
        self._maps = {}

    @classmethod
    def from_dict(cls, calib: dict, sensor_size: Tuple[int, int] = None, new_K=None, iterations: int = 20) -> Optional["CameraCalibration"]:
        """From the dict ``load_calib`` returns.  ``K`` or ``D`` being None is "no calibration", as the reference's loaders answer:
        the result is None."""
        if calib is None or calib.get("K") is None or calib.get("D") is None:
            return None
        if sensor_size is None:
            sensor_size = calib.get("sensor_size")
        return cls(calib["K"], calib["D"], sensor_size, calib.get("new_K") if new_K is None else new_K, iterations)

    def as_dict(self) -> dict:
        """{"K", "D"}: what the reference's ``load_calib`` documents."""
        return {"K": self.K.copy(), "D": self.D.copy()}

    @property
    def coefficients(self) -> np.ndarray:
        """(k1, k2, p1, p2, k3, k4, k5, k6), absent ones zero."""
        d = np.zeros(8)
        d[:self.D.size] = self.D
        return d

    @property
    def has_lens(self) -> bool:
        """False where every coefficient is zero and ``new_K`` is ``K``: rectification is then the identity."""
        return bool(np.any(self.D != 0) or np.any(self.K != self.new_K))

    def camera_array(self) -> np.ndarray:
        """The 16 doubles the kernels take: fx, fy, cx, cy of K, the same of new_K, the eight coefficients."""
        k, n = self.K, self.new_K
        return np.ascontiguousarray(np.concatenate([[k[0, 0], k[1, 1], k[0, 2], k[1, 2]], [n[0, 0], n[1, 1], n[0, 2], n[1, 2]],
                                                    self.coefficients]), dtype=np.float64)

    # ------------------------------------------------------------------ host: the forward model
    def distort_points(self, points) -> np.ndarray:
        """The forward model on the host, numpy float64: rectified pixel positions ``[..., 2] = (row', col')`` under ``new_K`` ->
        their sensor positions ``(row, col)``."""
        p = np.asarray(points, dtype=np.float64)
        if p.shape[-1:] != (2,):
            raise ValueError(f"points must be [..., 2] = (row, col), got shape {p.shape}")
        k1, k2, p1, p2, k3, k4, k5, k6 = self.coefficients
        x = (p[..., 1] - self.new_K[0, 2]) / self.new_K[0, 0]
        y = (p[..., 0] - self.new_K[1, 2]) / self.new_K[1, 1]
        xx, yy = x * x, y * y
        r2 = xx + yy
        rad = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        a = (2.0 * x) * y
        dx = p1 * a + p2 * (r2 + 2.0 * xx)
        dy = p1 * (r2 + 2.0 * yy) + p2 * a
        u = self.K[0, 0] * (x * rad + dx) + self.K[0, 2]
        v = self.K[1, 1] * (y * rad + dy) + self.K[1, 2]
        return np.stack([v, u], axis=-1)

    # ------------------------------------------------------------------ device: the inverse, once per device
    def rectify_map(self, device=None) -> torch.Tensor:
        """float64 ``[H, W, 2]``: the rectified ``(row', col')`` of every sensor pixel, built by one kernel and cached per device."""
        lib = _hip.require_gpu()
        dev = default_device() if device is None else torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._maps:
            H, W = self.sensor_size
            out = torch.empty((H, W, 2), dtype=torch.float64, device=dev)
            cam = self.camera_array()
            with _hip.on_device(dev):
                check(lib.ebos_rectify_map_f64(cam.ctypes.data_as(C.c_void_p), self.iterations, H, W, out.data_ptr(), stream_ptr(dev)),
                      "ebos_rectify_map_f64")
            self._maps[dev] = out
        return self._maps[dev]


def _scratch(lib, n: int, dev: torch.device) -> torch.Tensor:
    return torch.empty(int(lib.ebos_rectify_scratch_bytes(n)), dtype=torch.uint8, device=dev)


def rectify_events_raw(col: torch.Tensor, row: torch.Tensor, t: torch.Tensor, pol: torch.Tensor, calib: CameraCalibration,
                       ticks_per_second: float = 1e6, dtype: torch.dtype = torch.float64) -> Tuple[torch.Tensor, int, int]:
    """Raw sensor columns on the GPU (col int16 = sensor x, row int16 = sensor y, t int32 / int64 ticks, pol bool / uint8: what
    ``RawEventStore.load_raw`` returns) -> ``(events, n_outside_sensor, n_outside_image)``.

    ``events`` is ``[m, 4] = (row', col', t / ticks_per_second, p)`` of ``dtype`` (float64 or float32) in stream order: the sub-pixel
    position of every event under ``calib``; ``t`` and ``p`` are what ``RawEventStore.load_event`` makes of the same columns.  An event
    is dropped and counted when its pixel lies outside the sensor (``n_outside_sensor``), or when its rectified position, in
    ``dtype``, is not inside ``0 <= row' < H, 0 <= col' < W`` (``n_outside_image``) -- the domain on which the warp's ``trunc`` lookup
    is valid.  One host read-back (the three counts)."""
    if not isinstance(calib, CameraCalibration):
        raise ValueError(f"calib must be a CameraCalibration, got {type(calib).__name__}")
    if dtype not in (torch.float64, torch.float32):
        raise ValueError(f"dtype must be torch.float64 or torch.float32, got {dtype}")
    cols = (col, row, t, pol)
    if not all(isinstance(c, torch.Tensor) and c.ndim == 1 for c in cols) or len({int(c.shape[0]) for c in cols}) != 1:
        raise ValueError("col, row, t and pol must be 1-D tensors of equal length")
    if col.dtype != torch.int16 or row.dtype != torch.int16 or t.dtype not in (torch.int32, torch.int64) \
            or pol.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"columns must be int16, int16, int32 | int64, bool | uint8, got {col.dtype}, {row.dtype}, {t.dtype}, {pol.dtype}")
    n = int(col.shape[0])
    if n > MAX_EVENTS:
        raise ValueError(f"{n} events exceed the {MAX_EVENTS} one call takes")
    if not float(ticks_per_second) > 0:
        raise ValueError(f"ticks_per_second must be positive, got {ticks_per_second!r}")
    lib = _hip.require_gpu()
    if not all(c.is_cuda and c.device == col.device for c in cols):
        raise ValueError("col, row, t and pol must be on one GPU")
    dev = col.device
    col, row, t, pol = (c.contiguous() for c in cols)
    if pol.dtype == torch.bool:
        pol = pol.view(torch.uint8)
    H, W = calib.sensor_size
    rmap = calib.rectify_map(dev)
    out = torch.empty((n, 4), dtype=dtype, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    scratch = _scratch(lib, n, dev)
    with _hip.on_device(dev):
        check(lib.ebos_rectify_events_raw(_ptr(col), _ptr(row), _ptr(t), int(t.dtype == torch.int64), _ptr(pol), n, float(ticks_per_second),
                                          rmap.data_ptr(), H, W, H, W, int(dtype == torch.float32), _ptr(out), counts.data_ptr(),
                                          scratch.data_ptr(), scratch.numel(), stream_ptr(dev)), "ebos_rectify_events_raw")
    m, n_sensor = (int(v) for v in counts.cpu().numpy())
    return out[:m], n_sensor, n - m - n_sensor


def undistort_events(events, map_x, map_y, h: int, w: int):
    """The reference's ``undistort_events`` (src/utils/event_utils.py:242-266) on the GPU: ``k = int32(map_y[int32(x), int32(y)])``,
    ``l = int32(map_x[int32(x), int32(y)])`` (truncation toward zero), columns 0 and 1 of ``events`` ``[n, 4]`` replaced by ``k`` and
    ``l``, rows with ``0 <= k < h and 0 <= l < w`` kept in order.  numpy in -> numpy out, a CPU tensor in -> a CPU tensor out, a
    device tensor in -> a device tensor.  Like numpy's indexing, an event whose ``int32(x)``, ``int32(y)`` lie outside the maps
    raises ``IndexError`` (negative indices count from the end)."""
    if not isinstance(events, (np.ndarray, torch.Tensor)):
        raise ValueError(f"events must be a numpy array or a torch tensor, got {type(events).__name__}")
    if events.ndim != 2 or events.shape[1] != 4:
        raise ValueError(f"events must be [n, 4], got shape {tuple(events.shape)}")
    shapes = []
    for name, m in (("map_x", map_x), ("map_y", map_y)):
        if not isinstance(m, (np.ndarray, torch.Tensor)) or m.ndim != 2 or min(m.shape) < 1:
            raise ValueError(f"{name} must be a non-empty 2-D array (a meshgrid over the sensor), got "
                             f"{tuple(m.shape) if hasattr(m, 'shape') else type(m).__name__}")
        shapes.append(tuple(int(v) for v in m.shape))
    if shapes[0] != shapes[1]:
        raise ValueError(f"map_x {shapes[0]} and map_y {shapes[1]} must have one shape")
    if int(h) != h or int(w) != w or h < 0 or w < 0:
        raise ValueError(f"h and w must be non-negative integers, got {h!r}, {w!r}")
    numpy_in = isinstance(events, np.ndarray)
    dt = events.dtype if not numpy_in else (torch.float32 if events.dtype == np.float32 else torch.float64)
    if dt not in (torch.float32, torch.float64):
        dt = torch.float64
    n = int(events.shape[0])
    if n > MAX_EVENTS:
        raise ValueError(f"{n} events exceed the {MAX_EVENTS} one call takes")
    lib = _hip.require_gpu()
    on_gpu = not numpy_in and events.is_cuda
    dev = events.device if on_gpu else default_device()
    ev = (torch.from_numpy(np.ascontiguousarray(events)) if numpy_in else events).to(device=dev, dtype=dt).contiguous()
    mx, my = ((torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m).to(device=dev, dtype=torch.float64).contiguous()
              for m in (map_x, map_y))
    out = torch.empty_like(ev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    scratch = _scratch(lib, n, dev)
    fn = lib.ebos_undistort_events_f32 if dt == torch.float32 else lib.ebos_undistort_events_f64
    with _hip.on_device(dev):
        check(fn(_ptr(ev), n, mx.data_ptr(), my.data_ptr(), shapes[0][0], shapes[0][1], int(h), int(w), _ptr(out), counts.data_ptr(),
                 scratch.data_ptr(), scratch.numel(), stream_ptr(dev)), "ebos_undistort_events")
    m, bad = (int(v) for v in counts.cpu().numpy())
    if bad:
        raise IndexError(f"{bad} events index outside the {shapes[0][0]} x {shapes[0][1]} maps")
    res = out[:m]
    if numpy_in:
        return res.cpu().numpy().astype(events.dtype, copy=False)
    return res if on_gpu else res.cpu().to(events.dtype)
