"""Frame-based optical flow on the GPU (reference: src/frame_flow_estimator.py:30-95, ``FrameFlowEstimator``, and
src/utils/frame_utils.py:117-139,160-183, ``pad_to_same_resolution`` and ``bos_optical_flow``): the flow between camera frames that
the reference's driver scores every event-based estimate against (bos_event.py:155, 210-218).

The reference calls ``cv2.calcOpticalFlowFarneback`` with the YAML's ``params_opencv_flow`` on the host.  Here the same algorithm
(OpenCV 4.x's CPU path, flags 0) runs as HIP kernels, a batch of frame pairs per call (csrc/farneback.hip): per pyramid level a
level image of every frame, its polynomial expansion, the starting matrices and one fused window-sum / solve / matrix update per
iteration.  tests/_farneback_ref.py restates the algorithm in numpy; the kernels perform its float32 operations in its order, and the
float64 window sums in another order.  OpenCV is not available where this package is developed, so agreement with OpenCV's own
bits is not checked.

``calc_optical_flow_farneback`` follows cv2's argument order and layout ([H, W, 2] float32, channel 0 = the column displacement);
``farneback_batch`` returns a device [B, 2, H, W] (the reference's transposed layout) without a host synchronisation;
``bos_optical_flow``, ``pad_to_same_resolution`` and ``FrameFlowEstimator`` carry the reference's names and semantics.

Input rules (as in ``poisson``): numpy in -> numpy out, tensors in -> a device tensor out; views with a unit column stride (such as
the driver's ROI crop) are read in place; everything is validated before anything is uploaded.  Deliberate differences from the
reference: ``flags`` other than 0 raise ``NotImplementedError``; both frames of a pair must share one dtype (uint8, float32 or
float64); there is no CPU computation -- without a GPU the calls raise ``HipUnavailableError``.
"""
from __future__ import annotations

import logging
from typing import Sequence, Optional

import numpy as np
import torch

from . import _hip
from ._hip import check, stream_ptr
from ._staging import default_device

logger = logging.getLogger(__name__)

_DTYPES = {torch.uint8: _hip.FARNEBACK_U8, torch.float32: _hip.FARNEBACK_F32, torch.float64: _hip.FARNEBACK_F64}
PARAM_KEYS = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags")


def _dtype_of(x) -> torch.dtype:
    return x.dtype if isinstance(x, torch.Tensor) else torch.from_numpy(np.zeros(0, dtype=x.dtype)).dtype


def _check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags) -> tuple:
    if not 0 < pyr_scale < 1:
        raise ValueError(f"pyr_scale must lie in (0, 1), got {pyr_scale}")
    if int(levels) != levels or levels < 0:
        raise ValueError(f"levels must be a non-negative integer, got {levels}")
    if int(winsize) != winsize or winsize < 1:
        raise ValueError(f"winsize must be an integer >= 1, got {winsize}")
    if int(iterations) != iterations or iterations < 1:
        raise ValueError(f"iterations must be an integer >= 1, got {iterations}")
    if poly_n not in (5, 7):
        raise ValueError(f"poly_n must be 5 or 7, got {poly_n}")
    if not np.isfinite(poly_sigma):
        raise ValueError(f"poly_sigma must be finite, got {poly_sigma}")
    if flags != 0:
        raise NotImplementedError(f"flags {flags} are not supported: only 0 (OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN "
                                  "are out of scope)")
    return float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n), float(poly_sigma), 0


def _params_of(params: dict) -> tuple:
    missing = [k for k in PARAM_KEYS if k not in params]
    if missing:
        raise ValueError(f"params lacks {missing} (the keys of the YAML's params_opencv_flow)")
    return _check_params(*(params[k] for k in PARAM_KEYS))


def _check_frames(x, name: str, ndim: int):
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(x).__name__}")
    if x.ndim != ndim:
        raise ValueError(f"{name} must have {ndim} dimensions, got shape {tuple(x.shape)}")
    if _dtype_of(x) not in _DTYPES:
        raise ValueError(f"{name} must be uint8, float32 or float64, got {x.dtype}")
    if x.shape[-2] < 2 or x.shape[-1] < 2:
        raise ValueError(f"{name} frames must be at least 2 x 2, got {tuple(x.shape[-2:])}")


def _upload(x, device: Optional[torch.device]) -> torch.Tensor:
    """A device view the kernels read in place (unit column stride, non-negative strides), else a copy."""
    if isinstance(x, np.ndarray):
        if any(s < 0 for s in x.strides) or x.strides[-1] != x.itemsize:
            x = np.ascontiguousarray(x)
        x = torch.from_numpy(x)
    if not x.is_cuda:
        x = x.to(device or default_device())
    elif device is not None and x.device != device:
        x = x.to(device)
    if x.stride(-1) != 1 or any(s < 0 for s in x.stride()):
        x = x.contiguous()
    return x


def _launch(prev: torch.Tensor, next: torch.Tensor, p: tuple, out: torch.Tensor, out_strides: tuple) -> None:
    """prev [1 | B, H, W], next [B, H, W] device views of one dtype; out: a float32 device tensor whose storage holds the flow of
    pair b at (y, x) at element offsets b sb + y sr + x sx (dx) and + sc (dy) from out.data_ptr()."""
    lib = _hip.require_gpu()
    B, H, W = (int(v) for v in next.shape)
    shared = prev.shape[0] == 1
    dev = next.device
    scratch = torch.empty(int(lib.ebos_farneback_scratch_bytes(B, H, W, int(shared))), dtype=torch.uint8, device=dev)
    pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags = p
    sb, sc, sr, sx = out_strides
    with _hip.on_device(dev):
        check(lib.ebos_farneback(_DTYPES[next.dtype], B, H, W, prev.data_ptr(), 0 if shared else prev.stride(0), prev.stride(1),
                                 next.data_ptr(), next.stride(0), next.stride(1), pyr_scale, levels, winsize, iterations, poly_n,
                                 poly_sigma, flags, out.data_ptr(), sb, sc, sr, sx, scratch.data_ptr(), scratch.numel(),
                                 stream_ptr(dev)), "ebos_farneback")


def _prepare_pairs(prev, next, p_dims: int):
    """Validate and upload a batch: prev [B | 1, H, W] (or [H, W] with p_dims 2), next [B, H, W] -> device views."""
    _check_frames(prev, "prev", p_dims)
    _check_frames(next, "next", p_dims)
    if p_dims == 2:
        prev, next = prev[None], next[None]
    if next.shape[0] == 0:
        raise ValueError("next holds no frames")
    if tuple(prev.shape[1:]) != tuple(next.shape[1:]) or prev.shape[0] not in (1, next.shape[0]):
        raise ValueError(f"prev {tuple(prev.shape)} and next {tuple(next.shape)} must be [B | 1, H, W] and [B, H, W]")
    if _dtype_of(prev) != _dtype_of(next):
        raise ValueError(f"prev ({prev.dtype}) and next ({next.dtype}) must share one dtype")
    dev = next.device if isinstance(next, torch.Tensor) and next.is_cuda else (
        prev.device if isinstance(prev, torch.Tensor) and prev.is_cuda else None)
    nx = _upload(next, dev)
    pv = _upload(prev, nx.device)
    return pv, nx


def farneback_batch(prev, next, params: dict) -> torch.Tensor:
    """The flow of every pair (prev[b] or the shared prev[0], next[b]) in one call, without a host synchronisation.

    Args:
        prev ... [B, H, W] or [1, H, W] (one frame shared by all pairs) uint8 / float32 / float64, numpy or torch.
        next ... [B, H, W] of prev's dtype.
        params ... the YAML's params_opencv_flow: pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags (other keys
            are ignored).

    Returns:
        flow: device [B, 2, H, W] float32, component 0 = dx (columns), 1 = dy (rows): ``opencv_farneback``'s transposed layout.
    """
    p = _params_of(params)
    pv, nx = _prepare_pairs(prev, next, 3)
    B, H, W = (int(v) for v in nx.shape)
    out = torch.empty((B, 2, H, W), dtype=torch.float32, device=nx.device)
    _launch(pv, nx, p, out, tuple(out.stride()))
    return out


def calc_optical_flow_farneback(prev, next, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags=0):
    """cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags) for one
    pair of [H, W] frames -> [H, W, 2] float32 (dx, dy) with ``prev(y, x) ~ next(y + dy, x + dx)``.  numpy in -> numpy out;
    tensors in -> a device tensor."""
    p = _check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    numpy_out = not (isinstance(prev, torch.Tensor) or isinstance(next, torch.Tensor))
    pv, nx = _prepare_pairs(prev, next, 2)
    H, W = (int(v) for v in nx.shape[1:])
    out = torch.empty((H, W, 2), dtype=torch.float32, device=nx.device)
    _launch(pv, nx, p, out, (0, 1, 2 * W, 2))
    return out.cpu().numpy() if numpy_out else out


def bos_optical_flow(frame_a, frame_b, config: dict):
    """src/utils/frame_utils.py:160-183: ``cv2.calcOpticalFlowFarneback`` with the params of ``config`` -> [H, W, 2] float32."""
    p = _params_of(config)
    return calc_optical_flow_farneback(frame_a, frame_b, *p)


def pad_to_same_resolution(array, pad_config: dict, constant_value: float = 0.0):
    """src/utils/frame_utils.py:117-139: pad the last two axes by (pad_x0, pad_x1) rows and (pad_y0, pad_y1) columns with
    ``constant_value``; numpy arrays and torch tensors (on any device)."""
    if isinstance(array, torch.Tensor):
        pad = (pad_config["pad_y0"], pad_config["pad_y1"], pad_config["pad_x0"], pad_config["pad_x1"])
        return torch.nn.functional.pad(array, pad, mode="constant", value=constant_value)
    if isinstance(array, np.ndarray):
        pad = [(0, 0)] * array.ndim
        pad[-2] = (pad_config["pad_x0"], pad_config["pad_x1"])
        pad[-1] = (pad_config["pad_y0"], pad_config["pad_y1"])
        return np.pad(array, tuple(pad), constant_values=constant_value)
    return None   # (the reference falls through for anything else)


def _pads(params: dict) -> tuple:
    x0, x1, y0, y1 = (int(params[k]) for k in ("pad_x0", "pad_x1", "pad_y0", "pad_y1"))
    if min(x0, x1, y0, y1) < 0:
        raise ValueError(f"negative padding {(x0, x1, y0, y1)}")
    return x0, x1, y0, y1


def _padded_out(B: int, H: int, W: int, pads: tuple, device) -> tuple:
    """A zero [B, 2, H + pad_x0 + pad_x1, W + pad_y0 + pad_y1] tensor and the view of its ROI."""
    x0, x1, y0, y1 = pads
    full = torch.zeros((B, 2, H + x0 + x1, W + y0 + y1), dtype=torch.float32, device=device)
    return full, full[:, :, x0:x0 + H, y0:y0 + W]


class FrameFlowEstimator(object):
    """src/frame_flow_estimator.py:26-95 on the GPU: the frame-based flow of the driver's ``evaluate_per_frames``."""

    def __init__(self, visualizer_module=None) -> None:
        self.visualizer = visualizer_module

    def estimate(self, method: str, frame0, frame1, frame2, config: dict):
        if method == "opencv_flow":
            return self.opencv_farneback(frame1, frame2, config["params_opencv_flow"], visualize_frame=False)
        elif method == "opencv_flow_two_steps":
            return self.opencv_farneback_two_step(frame0, frame1, frame2, config["params_opencv_flow"])
        elif method == "openpiv":
            e = "openpiv is not supported by this package (OpenPIV runs on the host); use opencv_flow or opencv_flow_two_steps"
            logger.error(e)
            raise NotImplementedError(e)
        e = f"{method} is not supported"
        logger.error(e)
        raise NotImplementedError(e)

    def estimate_batch(self, method: str, frame0, frames, first: Sequence[int], second: Sequence[int], config: dict) -> torch.Tensor:
        """``estimate(method, frame0, frames[first[b]], frames[second[b]], config)`` for every pair b, on the device -> float32
        [B, 2, H + pads, W + pads] without a host synchronisation.  ``frames``: [n, H, W] (numpy or torch; a crop view is read in
        place), every distinct frame once; ``frame0``: the background [H, W], read by ``opencv_flow_two_steps`` only.  One Farneback
        chain for all pairs; two-step: the background against every distinct frame in one chain, one ``poisson_image`` of those
        flows, then the pairs' pictures against each other."""
        if method not in ("opencv_flow", "opencv_flow_two_steps"):
            return self.estimate(method, frame0, None, None, config)   # (raises as ``estimate`` does)
        params = config["params_opencv_flow"]
        p, pads = _params_of(params), _pads(params)
        _check_frames(frames, "frames", 3)
        if len(first) != len(second) or len(first) == 0:
            raise ValueError(f"first ({len(first)}) and second ({len(second)}) must name the same, non-zero number of pairs")
        fr = _upload(frames, frames.device if isinstance(frames, torch.Tensor) and frames.is_cuda else None)
        dev = fr.device
        i1, i2 = torch.as_tensor(list(first), device=dev), torch.as_tensor(list(second), device=dev)
        n, H, W = (int(v) for v in fr.shape)
        if method == "opencv_flow":
            full, roi = _padded_out(len(first), H, W, pads, dev)
            _launch(fr[i1], fr[i2], p, roi, tuple(roi.stride()))
            return full
        from .poisson import poisson_image

        _check_frames(frame0, "frame0", 2)
        if tuple(frame0.shape) != (H, W) or _dtype_of(frame0) != _dtype_of(fr):
            raise ValueError(f"frame0 {tuple(frame0.shape)} {frame0.dtype} differs from the frames {(H, W)} {fr.dtype}")
        f0 = _upload(frame0, dev)
        full, roi = _padded_out(n, H, W, pads, dev)
        _launch(f0[None].contiguous(), fr.contiguous(), p, roi, tuple(roi.stride()))
        pics = poisson_image(full)                                   # [n, Hf, Wf] uint8
        Hf, Wf = (int(v) for v in pics.shape[1:])
        out = torch.empty((len(first), 2, Hf, Wf), dtype=torch.float32, device=dev)
        _launch(pics[i1], pics[i2], p, out, tuple(out.stride()))
        return out

    def opencv_farneback_two_step(self, frame0, frame1, frame2, params_opencv_flow):
        """The background frame0 against frame1 and frame2 (one batch, frame0 shared), both flows integrated to their uint8
        Poisson pictures, then the flow between the pictures: [2, H + pads, W + pads], the second flow unpadded as in the
        reference."""
        from .poisson import poisson_image

        p, pads = _params_of(params_opencv_flow), _pads(params_opencv_flow)
        numpy_out = not any(isinstance(f, torch.Tensor) for f in (frame0, frame1, frame2))
        _check_frames(frame0, "frame0", 2)
        for name, f in (("frame1", frame1), ("frame2", frame2)):
            _check_frames(f, name, 2)
            if tuple(f.shape) != tuple(frame0.shape) or _dtype_of(f) != _dtype_of(frame0):
                raise ValueError(f"{name} {tuple(f.shape)} {f.dtype} differs from frame0 {tuple(frame0.shape)} {frame0.dtype}")
        dev = next((f.device for f in (frame1, frame2, frame0) if isinstance(f, torch.Tensor) and f.is_cuda), None)
        f1, f2 = _upload(frame1, dev), _upload(frame2, dev)
        dev = f1.device
        f0 = _upload(frame0, dev)
        if f2.device != dev:
            f2 = f2.to(dev)
        nx = torch.stack([f1, f2])
        H, W = (int(v) for v in nx.shape[1:])
        full, roi = _padded_out(2, H, W, pads, dev)
        _launch(f0[None], nx, p, roi, tuple(roi.stride()))
        pics = poisson_image(full)                                   # [2, Hf, Wf] uint8: p01, p02
        Hf, Wf = (int(v) for v in pics.shape[1:])
        out = torch.empty((1, 2, Hf, Wf), dtype=torch.float32, device=dev)
        _launch(pics[0:1], pics[1:2], p, out, tuple(out.stride()))
        return out[0].cpu().numpy() if numpy_out else out[0]

    def opencv_farneback(self, frame1, frame2, params_opencv_flow, visualize_frame=False):
        """The flow from frame1 to frame2, transposed to [2, H, W] and zero-padded to the full frame by the params' pad_*."""
        p, pads = _params_of(params_opencv_flow), _pads(params_opencv_flow)
        numpy_out = not (isinstance(frame1, torch.Tensor) or isinstance(frame2, torch.Tensor))
        pv, nx = _prepare_pairs(frame1, frame2, 2)
        H, W = (int(v) for v in nx.shape[1:])
        full, roi = _padded_out(1, H, W, pads, nx.device)
        _launch(pv, nx, p, roi, tuple(roi.stride()))
        if visualize_frame and self.visualizer is not None:
            f_next = roi[0].permute(1, 2, 0).cpu().numpy()
            self.visualizer.visualize_optical_flow(f_next[..., 0], f_next[..., 1], file_prefix="frame_flow_concurrent")
            self.visualizer.visualize_image(_host(frame1), file_prefix="frame_current")
            self.visualizer.visualize_image(_host(frame2), file_prefix="frame_next")
        return full[0].cpu().numpy() if numpy_out else full[0]


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x
