"""Camera frames warped into the event view on the GPU (reference: src/data_loader/ccs.py:373-396, ``CcsDataLoader.load_image``
with ``data.warp: true`` -> ``cv2.warpPerspective(image, homography, (W, H))``, and the driver's crop, bos_event.py:25-39,
``validate_image``).

The reference warps every frame on the host with OpenCV and crops it afterwards.  Here a batch of frames is warped by one launch
of csrc/frame_warp.hip, which can compute the crop's rectangle alone and write it where the frame-flow kernels and the generative
solvers read it in place.  The arithmetic is OpenCV's classic fixed-point ``warpPerspective`` (4.5 - 4.10) as
tests/_warp_ref.py restates it in numpy; the kernel agrees with that restatement bit for bit for uint8 frames.  It restates
OpenCV's classic algorithm and is not checked against OpenCV, which is absent where this package is developed; OpenCV >= 4.11's
newer linear path may differ in the last grey level.

``warp_perspective`` follows cv2's argument order (``dsize`` = (W, H)); ``warp_perspective_batch`` takes [B, Hs, Ws] and one
matrix or one per frame and does no host synchronisation.  ``roi`` = (xmin, xmax, ymin, ymax) names destination ROWS
[xmin, xmax) and COLUMNS [ymin, ymax), the reference's ``common_params`` convention (a dict with those keys is accepted).

Input rules (as in ``frame_flow`` and ``poisson``): numpy in -> numpy out, tensors in -> a device tensor out; everything is
validated before anything is uploaded.  ``M`` is host data (a device tensor is copied to the host, which synchronises).
Deliberate differences from cv2: single-channel uint8 or float32 frames only; INTER_NEAREST and INTER_LINEAR with BORDER_CONSTANT
only (other flags raise ``NotImplementedError``); a singular matrix raises ``ValueError``; there is no CPU computation -- without a
GPU the calls raise ``HipUnavailableError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip
from ._hip import check, stream_ptr
from ._staging import default_device

INTER_NEAREST = 0
INTER_LINEAR = 1
WARP_INVERSE_MAP = 16

_DTYPES = {torch.uint8: _hip.WARP_U8, torch.float32: _hip.WARP_F32}
_MAX_SOURCE, _MAX_DEST, _MAX_ENTRY = 32767, 65535, 1e100
Roi = Union[Sequence[int], dict]


def _dtype_of(x) -> torch.dtype:
    return x.dtype if isinstance(x, torch.Tensor) else torch.from_numpy(np.zeros(0, dtype=x.dtype)).dtype


def _check_frames(x, name: str, ndim: int) -> None:
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(x).__name__}")
    if x.ndim != ndim:
        raise ValueError(f"{name} must have {ndim} dimensions, got shape {tuple(x.shape)}")
    try:
        ok = _dtype_of(x) in _DTYPES
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"{name} must be uint8 or float32, got {x.dtype}")
    if min(x.shape) < 1 or x.shape[-2] > _MAX_SOURCE or x.shape[-1] > _MAX_SOURCE:
        raise ValueError(f"{name} frames must be 1 .. {_MAX_SOURCE} pixels a side and the batch non-empty, got {tuple(x.shape)}")


def _check_flags(flags) -> int:
    try:
        ok = int(flags) == flags and (int(flags) & ~WARP_INVERSE_MAP) in (INTER_NEAREST, INTER_LINEAR)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise NotImplementedError(f"flags {flags} are not supported: only INTER_NEAREST (0) or INTER_LINEAR (1), optionally "
                                  "| WARP_INVERSE_MAP (16), with BORDER_CONSTANT")
    return int(flags)


def _det3(m: np.ndarray) -> float:
    return m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) \
        + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])


def _check_matrix(M, B: Optional[int], flags: int) -> np.ndarray:
    """-> contiguous float64 [3, 3] or [B, 3, 3]."""
    if isinstance(M, torch.Tensor):
        M = M.detach().cpu().numpy()
    try:
        m = np.ascontiguousarray(M, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise ValueError(f"M must be a 3 x 3 matrix of numbers: {err}") from None
    if m.shape != (3, 3) and (B is None or m.shape != (B, 3, 3)):
        raise ValueError(f"M must be 3 x 3" + ("" if B is None else f" or {B} x 3 x 3") + f", got {m.shape}")
    if not np.isfinite(m).all() or np.abs(m).max() > _MAX_ENTRY:
        raise ValueError("M has entries that are not finite (or beyond 1e100)")
    if not flags & WARP_INVERSE_MAP:
        for k, one in enumerate(m.reshape(-1, 3, 3)):
            with np.errstate(over="ignore", invalid="ignore"):
                det = _det3(one)
            if det == 0 or not np.isfinite(det):
                raise ValueError(f"M{'' if m.ndim == 2 else f'[{k}]'} is singular")
    return m


def _check_dsize(dsize) -> Tuple[int, int]:
    try:
        W, H = dsize
        ok = int(W) == W and int(H) == H and 0 < W <= _MAX_DEST and 0 < H <= _MAX_DEST
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"dsize must be (W, H) with 1 .. {_MAX_DEST} pixels a side, got {dsize!r}")
    return int(W), int(H)


def _check_roi(roi: Optional[Roi], H: int, W: int) -> Tuple[int, int, int, int]:
    if roi is None:
        return 0, H, 0, W
    try:
        r = tuple(roi[k] for k in ("xmin", "xmax", "ymin", "ymax")) if isinstance(roi, dict) else tuple(roi)
        ok = len(r) == 4 and all(int(v) == v for v in r)
    except (KeyError, TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"roi must be (xmin, xmax, ymin, ymax) or a dict with those keys, got {roi!r}")
    xmin, xmax, ymin, ymax = (int(v) for v in r)
    if not (0 <= xmin < xmax <= H and 0 <= ymin < ymax <= W):
        raise ValueError(f"roi rows [{xmin}, {xmax}) columns [{ymin}, {ymax}) must lie inside the {H} x {W} destination")
    return xmin, xmax, ymin, ymax


def _upload(x, device: Optional[torch.device]) -> torch.Tensor:
    """A device view the kernel reads in place (unit column stride, non-negative strides), else a copy."""
    if isinstance(x, np.ndarray):
        if any(s < 0 for s in x.strides) or x.strides[-1] != x.itemsize:
            x = np.ascontiguousarray(x)
        x = torch.from_numpy(x)
    if not x.is_cuda:
        x = x.to(device or default_device(), non_blocking=True)
    elif device is not None and x.device != device:
        x = x.to(device)
    if x.stride(-1) != 1 or any(s < 0 for s in x.stride()) or (x.shape[1] > 1 and x.stride(1) < x.shape[2]):
        x = x.contiguous()
    return x


def _launch(srcs: torch.Tensor, m: np.ndarray, H: int, W: int, flags: int, border_value: float, rect: tuple, out: torch.Tensor) -> None:
    """srcs: a device [B, Hs, Ws] view; out: a device [B, h, w] view of srcs' dtype with a unit column stride."""
    lib = _hip.require_gpu()
    B, Hs, Ws = (int(v) for v in srcs.shape)
    dev = srcs.device
    with _hip.on_device(dev):
        check(lib.ebos_warp_perspective(_DTYPES[srcs.dtype], B, Hs, Ws, srcs.data_ptr(), srcs.stride(0) if B > 1 else 0, srcs.stride(1),
                                        m.ctypes.data_as(C.c_void_p), 9 if m.ndim == 3 else 0, H, W, flags, float(border_value), *rect,
                                        out.data_ptr(), out.stride(0) if B > 1 else 0, out.stride(1), stream_ptr(dev)),
              "ebos_warp_perspective")


def _validate(srcs, ndim, M, dsize, flags, border_value, roi):
    _check_frames(srcs, "src" if ndim == 2 else "srcs", ndim)
    flags = _check_flags(flags)
    m = _check_matrix(M, None if ndim == 2 else int(srcs.shape[0]), flags)
    W, H = _check_dsize(dsize)
    rect = _check_roi(roi, H, W)
    try:
        border_value = float(border_value)
        ok = np.isfinite(border_value)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"border_value must be one finite number, got {border_value!r}")
    return flags, m, W, H, rect, border_value


def warp_perspective_batch(srcs, M, dsize, flags: int = INTER_LINEAR, border_value: float = 0, roi: Optional[Roi] = None,
                           out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """Every frame of ``srcs`` warped in one launch, without a host synchronisation.

    Args:
        srcs ... [B, Hs, Ws] uint8 / float32, numpy or torch (a host array is uploaded once, asynchronously where it is page-locked).
        M ... [3, 3] shared by the batch or [B, 3, 3] (host data), the source -> destination map unless WARP_INVERSE_MAP.
        dsize ... (W, H) of the destination, as in cv2.
        roi ... destination rows [xmin, xmax) and columns [ymin, ymax) to compute (``validate_image``'s crop); None = all.
        out ... optional device [B, h, w] view of srcs' dtype with a unit column stride (a slice of a larger tensor, say) to write into.

    Returns:
        device [B, h, w] of srcs' dtype (``out`` where given).
    """
    flags, m, W, H, rect, border_value = _validate(srcs, 3, M, dsize, flags, border_value, roi)
    B, h, w = int(srcs.shape[0]), rect[1] - rect[0], rect[3] - rect[2]
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (B, h, w) and out.dtype == _dtype_of(srcs)
                and out.stride(2) == 1 and out.stride(1) >= w and out.stride(0) >= 0):
            raise ValueError(f"out must be a device [{B}, {h}, {w}] tensor of {srcs.dtype} with a unit column stride")
        device = out.device
    dev = srcs.device if isinstance(srcs, torch.Tensor) and srcs.is_cuda else (torch.device(device) if device is not None else None)
    sv = _upload(srcs, dev)
    if out is None:
        out = torch.empty((B, h, w), dtype=sv.dtype, device=sv.device)
    elif out.device != sv.device:
        raise ValueError(f"out is on {out.device}, the frames on {sv.device}")
    _launch(sv, m, H, W, flags, border_value, rect, out)
    return out


def warp_perspective(src, M, dsize, flags: int = INTER_LINEAR, border_value: float = 0, roi: Optional[Roi] = None):
    """``cv2.warpPerspective(src, M, dsize, flags=flags, borderMode=BORDER_CONSTANT, borderValue=border_value)`` for one [Hs, Ws]
    uint8 / float32 frame -> [H, W] (or the rows and columns of ``roi``).  numpy in -> numpy out; a tensor in -> a device tensor."""
    flags, m, W, H, rect, border_value = _validate(src, 2, M, dsize, flags, border_value, roi)
    numpy_out = not isinstance(src, torch.Tensor)
    sv = _upload(src[None], src.device if not numpy_out and src.is_cuda else None)
    out = torch.empty((1, rect[1] - rect[0], rect[3] - rect[2]), dtype=sv.dtype, device=sv.device)
    _launch(sv, m, H, W, flags, border_value, rect, out)
    return out[0].cpu().numpy() if numpy_out else out[0]


def _check_calib(calib, Hs: int, Ws: int):
    from .calibration import CameraCalibration

    if not isinstance(calib, CameraCalibration):
        raise ValueError(f"calib must be a CameraCalibration, got {type(calib).__name__}")
    if calib.sensor_size != (Hs, Ws):
        raise ValueError(f"the calibration belongs to a {calib.sensor_size[0]} x {calib.sensor_size[1]} sensor, the frames are {Hs} x {Ws}")
    return calib


def _validate_undistort(srcs, ndim, calib, homography, dsize, roi, border_value):
    _check_frames(srcs, "image" if ndim == 2 else "images", ndim)
    Hs, Ws = int(srcs.shape[-2]), int(srcs.shape[-1])
    _check_calib(calib, Hs, Ws)
    m = None if homography is None else _check_matrix(homography, None, 0)
    W, H = (Ws, Hs) if dsize is None else _check_dsize(dsize)
    rect = _check_roi(roi, H, W)
    try:
        border_value = float(border_value)
        ok = np.isfinite(border_value)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"border_value must be one finite number, got {border_value!r}")
    return m, W, H, rect, border_value


def _launch_undistort(srcs: torch.Tensor, calib, m: Optional[np.ndarray], H: int, W: int, border_value: float, rect: tuple,
                      out: torch.Tensor) -> None:
    lib = _hip.require_gpu()
    B, Hs, Ws = (int(v) for v in srcs.shape)
    dev = srcs.device
    cam = calib.camera_array()
    fn = lib.ebos_undistort_image_u8 if srcs.dtype == torch.uint8 else lib.ebos_undistort_image_f32
    with _hip.on_device(dev):
        check(fn(B, Hs, Ws, srcs.data_ptr(), srcs.stride(0) if B > 1 else 0, srcs.stride(1), cam.ctypes.data_as(C.c_void_p),
                 None if m is None else m.ctypes.data_as(C.c_void_p), H, W, float(border_value), *rect, out.data_ptr(),
                 out.stride(0) if B > 1 else 0, out.stride(1), stream_ptr(dev)), "ebos_undistort_image")


def undistort_image_batch(images, calib, homography=None, dsize=None, roi: Optional[Roi] = None, border_value: float = 0,
                          out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """Every frame of ``images`` [B, Hs, Ws] (uint8 / float32, numpy or torch) rectified in one launch, without a host
    synchronisation: see ``undistort_image``.  ``out``: an optional device [B, h, w] view with a unit column stride to write into.
    Returns a device [B, h, w] tensor; a frame's bits do not depend on the batch it is in."""
    m, W, H, rect, border_value = _validate_undistort(images, 3, calib, homography, dsize, roi, border_value)
    B, h, w = int(images.shape[0]), rect[1] - rect[0], rect[3] - rect[2]
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (B, h, w) and out.dtype == _dtype_of(images)
                and out.stride(2) == 1 and out.stride(1) >= w and out.stride(0) >= 0):
            raise ValueError(f"out must be a device [{B}, {h}, {w}] tensor of {images.dtype} with a unit column stride")
        device = out.device
    dev = images.device if isinstance(images, torch.Tensor) and images.is_cuda else (torch.device(device) if device is not None else None)
    sv = _upload(images, dev)
    if out is None:
        out = torch.empty((B, h, w), dtype=sv.dtype, device=sv.device)
    elif out.device != sv.device:
        raise ValueError(f"out is on {out.device}, the frames on {sv.device}")
    _launch_undistort(sv, calib, m, H, W, border_value, rect, out)
    return out


def undistort_image(image, calib, homography=None, dsize=None, roi: Optional[Roi] = None, border_value: float = 0):
    """One [Hs, Ws] uint8 / float32 frame of the camera ``calib`` (a ``CameraCalibration`` whose ``sensor_size`` is the frame's)
    rectified -- ``cv2.undistort(image, K, D, None, new_K)`` -- and, where ``homography`` (3 x 3, rectified frame -> destination, as
    ``cv2.warpPerspective`` takes it) is given, warped into the destination ``dsize`` = (W, H) (default: the frame's own size) IN
    THE SAME RESAMPLE: an output pixel takes its ideal position (through the inverse homography), is normalised by ``new_K``, pushed
    through the lens model and sampled there with the fixed-point bilinear arithmetic of ``warp_perspective`` (constant border).
    One resample is not two: the result is not ``warp_perspective(undistort(image))`` pixel for pixel, it is sharper.  Where
    every coefficient of ``D`` is zero and ``new_K`` is ``K`` the result is ``warp_perspective``'s bit for bit.  ``roi`` as there.
    numpy in -> numpy out; a tensor in -> a device tensor.  Restated by tests/_rectify_ref.py; not checked against OpenCV."""
    m, W, H, rect, border_value = _validate_undistort(image, 2, calib, homography, dsize, roi, border_value)
    numpy_out = not isinstance(image, torch.Tensor)
    sv = _upload(image[None], image.device if not numpy_out and image.is_cuda else None)
    out = torch.empty((1, rect[1] - rect[0], rect[3] - rect[2]), dtype=sv.dtype, device=sv.device)
    _launch_undistort(sv, calib, m, H, W, border_value, rect, out)
    return out[0].cpu().numpy() if numpy_out else out[0]


def check_even_crop(h: int, w: int, roi) -> None:
    """The driver refuses a crop with an odd number of rows or columns (its later stages halve the frame): so does this."""
    if h % 2:
        raise AssertionError(f"the crop keeps {h} rows, an odd number: choose xmin / xmax an even distance apart ({roi})")
    if w % 2:
        raise AssertionError(f"the crop keeps {w} columns, an odd number: choose ymin / ymax an even distance apart ({roi})")


def validate_image(image, config: dict):
    """The driver's crop of a frame to the region of interest (reference: ``validate_image``, bos_event.py): rows
    ``config["xmin"] .. config["xmax"]`` and columns ``config["ymin"] .. config["ymax"]`` of the LAST two axes, so a single
    [H, W] frame and a [B, H, W] batch are cropped alike; numpy arrays and tensors; the result is a view.  Like the driver, it
    refuses (``AssertionError``) a crop whose row or column count is odd."""
    rows, cols = slice(config["xmin"], config["xmax"]), slice(config["ymin"], config["ymax"])
    cropped = image[..., rows, cols]
    check_even_crop(int(cropped.shape[-2]), int(cropped.shape[-1]), {k: config[k] for k in ("xmin", "xmax", "ymin", "ymax")})
    return cropped
