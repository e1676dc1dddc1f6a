"""The reference's flow-error metrics on the GPU (reference: src/utils/flow_utils.py:706-823): EPE, the share of pixels whose
end-point error exceeds 1, 2, 3, 5, 10 and 20 px (1PE ... 20PE) and the angular error AE, over the pixels where the ground truth
is valid (finite and non-zero in both components) and, optionally, an event mask.

``calculate_flow_error_numpy`` and ``calculate_flow_error_tensor`` have the reference's names, signatures and keys and give its
results, NaNs included: the kernel (csrc/flow_error.hip) repeats the reference's per-pixel IEEE operations in its order, without
FMA contraction, so for float64 flows every pixel's end-point error is bit-equal to numpy's and the counts are exact.  Sums are
float64 in one fixed order, so results are the same on every run.  ``flow_error_batch`` scores a whole batch in three launches with
no host synchronisation and returns the per-item table.

Deliberate differences from the reference:
  - the numpy variant returns ``np.float64`` values also for float32 inputs; the tensor variant returns 0-dim device tensors of
    the flow dtype (the reference's kPE of float64 tensors are float32, and its ``n`` is formed in float32, torch's default
    dtype: its tensor EPE / AE differ from the numpy variant's by up to 1e-5 / count relative; here both variants use the
    numpy variant's float64 ``n = count + 1e-5``);
  - float32 flows are masked, scaled and differenced in float32 as in the reference, but the norm, the AE term and the sums are
    float64 (the reference sums in float32);
  - inputs that do not fit the documented shapes raise ``ValueError`` instead of broadcasting into something else;
  - there is no CPU computation: numpy arrays and CPU tensors are uploaded, and without a GPU the call raises
    ``HipUnavailableError``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import check, stream_ptr
from ._staging import default_device

KEYS = ("EPE", "1PE", "2PE", "3PE", "5PE", "10PE", "20PE", "AE")
COLUMNS = KEYS + ("n_points",)   # the columns of flow_error_batch's table (n_points = count of the mask, without the 1e-5)
_DTYPES = {torch.float32: _hip.FLOW_ERROR_F32, torch.float64: _hip.FLOW_ERROR_F64}


def _as_tensor(x, name: str, device: Optional[torch.device]) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        if any(s < 0 for s in x.strides):
            x = np.ascontiguousarray(x)
        x = torch.from_numpy(x)
    elif not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(x).__name__}")
    if not x.is_cuda:
        x = x.to(device or default_device())
    return x


def _flow_view(f: torch.Tensor) -> torch.Tensor:
    """The flow as the kernel reads it: unit column stride (a view of an ROI keeps its row and batch strides)."""
    if f.stride(3) != 1 and f.shape[3] != 1:
        f = f.contiguous()
    return f


def _prepare(flow_gt, flow_pred, event_mask, time_scale):
    """-> (dtype code, gt, pred, mask uint8 [B, H, W] view or None, time_scale [B] or None), all on one device."""
    for name, f in (("flow_gt", flow_gt), ("flow_pred", flow_pred)):
        if not isinstance(f, (np.ndarray, torch.Tensor)):
            raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(f).__name__}")
        if f.ndim != 4:
            raise ValueError(f"{name} must be [B, 2, H, W], got shape {tuple(f.shape)}")
        floating = f.dtype.is_floating_point if isinstance(f, torch.Tensor) else np.issubdtype(f.dtype, np.floating)
        if not floating:
            raise ValueError(f"{name} must be a floating-point array, got {f.dtype}")
    if tuple(flow_gt.shape) != tuple(flow_pred.shape):
        raise ValueError(f"flow_gt {tuple(flow_gt.shape)} and flow_pred {tuple(flow_pred.shape)} differ in shape")
    B, C, H, W = (int(v) for v in flow_gt.shape)
    if C != 2 or B == 0 or H == 0 or W == 0:
        raise ValueError(f"flows must be [B, 2, H, W] with B, H, W > 0, got {tuple(flow_gt.shape)}")
    dev = flow_gt.device if isinstance(flow_gt, torch.Tensor) and flow_gt.is_cuda else (
        flow_pred.device if isinstance(flow_pred, torch.Tensor) and flow_pred.is_cuda else None)
    gt, pred = _as_tensor(flow_gt, "flow_gt", dev), _as_tensor(flow_pred, "flow_pred", dev)
    dev = gt.device
    if pred.device != dev:
        pred = pred.to(dev)
    dtype = torch.promote_types(gt.dtype, pred.dtype)
    if dtype not in _DTYPES:
        raise ValueError(f"flows must be float32 or float64, got {gt.dtype} / {pred.dtype}")
    gt, pred = _flow_view(gt.to(dtype)), _flow_view(pred.to(dtype))

    mask = None
    if event_mask is not None:
        m = _as_tensor(event_mask, "event_mask", dev)
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
        elif m.dtype != torch.uint8:
            m = (m != 0).view(torch.uint8)
        if m.dim() > 4:
            raise ValueError(f"event_mask of shape {tuple(m.shape)} does not broadcast to [B, 1, H, W] = {(B, 1, H, W)}")
        m = m.reshape((1,) * (4 - m.dim()) + tuple(m.shape))
        try:
            m = m.expand(B, 1, H, W)
        except RuntimeError:
            raise ValueError(f"event_mask of shape {tuple(event_mask.shape)} does not broadcast to [B, 1, H, W] = {(B, 1, H, W)}") from None
        mask = m[:, 0]
        if mask.stride(2) != 1 and W != 1:
            mask = mask.contiguous()

    ts = None
    if time_scale is not None:
        ts = torch.as_tensor(time_scale) if not isinstance(time_scale, torch.Tensor) else time_scale
        if ts.numel() != B:
            raise ValueError(f"time_scale must hold one value per item ({B}), got shape {tuple(ts.shape)}")
        ts = ts.to(device=dev, dtype=dtype).reshape(B).contiguous()
    return _DTYPES[dtype], gt, pred, mask, ts


def _launch(code, gt, pred, mask, ts, clamp: bool) -> torch.Tensor:
    lib = _hip.require_gpu()
    B, _, H, W = gt.shape
    dev = gt.device
    out = torch.empty((B + 1, len(COLUMNS)), dtype=torch.float64, device=dev)
    scratch = torch.empty(int(lib.ebos_flow_error_scratch_bytes(B, H, W)), dtype=torch.uint8, device=dev)
    m_sb, m_sr = (mask.stride(0), mask.stride(1)) if mask is not None else (0, 0)
    with _hip.on_device(dev):
        check(lib.ebos_flow_error(code, B, H, W, gt.data_ptr(), gt.stride(0), gt.stride(1), gt.stride(2),
                                  pred.data_ptr(), pred.stride(0), pred.stride(1), pred.stride(2),
                                  None if mask is None else mask.data_ptr(), m_sb, m_sr, None if ts is None else ts.data_ptr(),
                                  _hip.FLOW_ERROR_CLAMP_AE if clamp else 0, out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                  stream_ptr(dev)), "ebos_flow_error")
    return out


def flow_error_batch(flow_gt, flow_pred, event_mask=None, time_scale=None, *, clamp_angle: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Flow errors of every item of a batch in three launches, without a host synchronisation.

    Args:
        flow_gt, flow_pred ... [B, 2, H, W] float32 / float64 (numpy or torch; uploaded when not on the GPU).  Views with a unit
            column stride (an ROI such as ``flow[:, :, 0:720, 320:960]``) are read in place.
        event_mask ... optional, broadcasts to [B, 1, H, W]; any non-zero value counts.
        time_scale ... optional, B values multiplied into both masked flows (calculate_flow_error_tensor's).
        clamp_angle ... clamp the AE cosine to [-1, 1] (NOT the reference: its AE is NaN wherever rounding pushes the cosine
            above 1, which happens on many pixels of a near-perfect prediction).

    Returns:
        (per_item, means): float64 device tensors [B, 9] and [9], columns ``COLUMNS`` (EPE, 1PE, 2PE, 3PE, 5PE, 10PE, 20PE, AE,
        n_points); ``means`` is the mean over the batch of each column -- the reference's values.
    """
    code, gt, pred, mask, ts = _prepare(flow_gt, flow_pred, event_mask, time_scale)
    out = _launch(code, gt, pred, mask, ts, clamp_angle)
    return out[:-1], out[-1]


def calculate_flow_error_tensor(flow_gt: torch.Tensor, flow_pred: torch.Tensor, event_mask: Optional[torch.Tensor] = None,
                                time_scale: Optional[torch.Tensor] = None) -> dict:
    """src/utils/flow_utils.py:706-770.  flow_gt, flow_pred [B, 2, H, W]; event_mask broadcasting to [B, 1, H, W]; time_scale
    [B] (or [B, 1]) multiplied into both masked flows.  Returns {"EPE", "1PE", "2PE", "3PE", "5PE", "10PE", "20PE", "AE"}: 0-dim
    device tensors of the flow dtype, each the mean over the batch."""
    code, gt, pred, mask, ts = _prepare(flow_gt, flow_pred, event_mask, time_scale)
    means = _launch(code, gt, pred, mask, ts, False)[-1].to(gt.dtype)
    return {k: means[i] for i, k in enumerate(KEYS)}


def calculate_flow_error_numpy(flow_gt: np.ndarray, flow_pred: np.ndarray, event_mask: Optional[np.ndarray] = None) -> dict:
    """src/utils/flow_utils.py:773-823.  flow_gt, flow_pred [B, 2, H, W]; event_mask broadcasting to [B, 1, H, W] (a device
    tensor is accepted too and stays on the device).  Returns the reference's keys with ``np.float64`` values (one read-back)."""
    code, gt, pred, mask, ts = _prepare(flow_gt, flow_pred, event_mask, None)
    means = _launch(code, gt, pred, mask, ts, False)[-1].cpu().numpy()
    return {k: np.float64(means[i]) for i, k in enumerate(KEYS)}
