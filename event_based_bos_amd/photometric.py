"""Does a flow explain the two camera frames it was estimated between?  The reference's frame warp and SSIM on the GPU, and a fused
per-item score built from them (csrc/photometric.hip).

``warp_image_forward`` and ``warp_image_torch`` (reference: src/utils/frame_utils.py:56-115) sample an image at ``x - flow``
through the reference's chain -- a float32 base grid, the displacement subtracted in its own type, ``grid_sample``'s
``align_corners=True`` un-normalisation, four taps with zeros outside -- and ``ssim`` / ``SSIM`` (src/utils/stat_utils.py:215-285)
evaluate the reference's SSIM map under its own 11 x 11 taps, which the host forms exactly as ``create_window`` does.  The kernels
repeat the reference's operations without FMA contraction; their results differ from the reference's by the order of the window
sums alone.  ``photometric_error_batch`` scores a batch in two launches with no host synchronisation: per item the mean absolute
difference, the root mean square difference and the mean SSIM between ``warp_image_forward(frame1, flow)`` and ``frame2`` over the
counted pixels, the same three for the un-warped ``frame1`` as a baseline, and the count.  A pixel is counted when it lies in the
``roi``, the ``mask`` is non-zero there, the flow is finite there and all four of its bilinear taps lie inside the image.

Deliberate differences from the reference:
  - forward only: an input that requires grad raises ``ValueError``;
  - inputs that do not fit the documented shapes raise ``ValueError`` instead of broadcasting into something else;
  - the two images of an SSIM pair, and a float image and its flow, must share a dtype (uint8 images go with any flow);
  - ``warp_image_torch`` converts its image to float64 (the reference's grid is float64 and takes no other image);
  - the means of ``ssim`` and of the score are the exact float64 sums rounded once (the kernels carry every sum as a pair hi + lo),
    divided, and for ``ssim`` cast to the input dtype: they do not depend on the order of summation (the reference's ``mean`` sums
    in the input dtype, in an order that depends on the thread count);
  - window sizes above ``max_window_size()`` (13) are not built;
  - there is no CPU computation: numpy arrays and CPU tensors are uploaded, and without a GPU the call raises
    ``HipUnavailableError``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import check, ptr, stream_ptr
from ._staging import default_device

COLUMNS = ("L1", "RMSE", "SSIM", "L1_0", "RMSE_0", "SSIM_0", "n_points")
_CODES = {torch.uint8: _hip.IMAGE_U8, torch.float32: _hip.IMAGE_F32, torch.float64: _hip.IMAGE_F64}
_FLOATS = (torch.float32, torch.float64)


def max_window_size() -> int:
    """The largest SSIM window the kernels are built for."""
    return int(_hip.load_library().ebos_photometric_max_window())


def window_taps(window_size: int = 11, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The reference's ``create_window`` (src/utils/stat_utils.py:216-225) on the host: the 1-D Gaussian (sigma 1.5) as a float32
    tensor, normalised in float32, the outer product in float32, then cast to ``dtype`` -> [window_size, window_size]."""
    window_size = _window(window_size)
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().to(dtype).contiguous()


def _window(window_size) -> int:
    if isinstance(window_size, bool) or int(window_size) != window_size or int(window_size) < 1 or int(window_size) % 2 == 0:
        raise ValueError(f"window_size must be a positive odd integer, got {window_size!r}")
    return int(window_size)


def _check_array(x, name: str):
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(x).__name__}")
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise ValueError(f"{name} requires grad: the photometric functions are forward only")
    return x


def _torch(x) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x))
    return x.detach()


def _device_of(*xs) -> Optional[torch.device]:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return None


def _upload(x: torch.Tensor, device: torch.device, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    if x.device != device:
        x = x.to(device)
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    return x.contiguous()


def _image_shape(image, name: str) -> Tuple[int, int]:
    H, W = (int(v) for v in image.shape[-2:])
    if H < 2 or W < 2:
        raise ValueError(f"{name} must be at least 2 x 2 (the base grid divides by (size - 1) / 2), got {H} x {W}")
    return H, W


# ------------------------------------------------------------------------------------------------ the warp
def _warp_launch(images: torch.Tensor, shared: bool, flows: Optional[torch.Tensor], shifts: Optional[torch.Tensor],
                 compute: torch.dtype, B: int, H: int, W: int) -> torch.Tensor:
    """images [B or 1, H, W] uint8 or ``compute``; flows [B, 2, H, W] of ``compute`` or shifts [B, 2]; all on one device."""
    lib = _hip.require_gpu()
    dev = images.device
    out = torch.empty((B, H, W), dtype=compute, device=dev)
    fn = lib.ebos_warp_image_forward_f64 if compute == torch.float64 else lib.ebos_warp_image_forward_f32
    with _hip.on_device(dev):
        check(fn(images.data_ptr(), _CODES[images.dtype], 0 if shared else H * W, ptr(flows), ptr(shifts),
                 _CODES[shifts.dtype] if shifts is not None else 0, B, H, W, out.data_ptr(), stream_ptr(dev)), "ebos_warp_image_forward")
    return out


def _warp_inputs(images, flows, image_dims: str):
    """Validated (images tensor, flows tensor, shared, B, H, W, compute dtype) of a batched warp; nothing uploaded yet."""
    images, flows = _torch(_check_array(images, "images")), _torch(_check_array(flows, "flows"))
    if flows.dim() != 4 or flows.shape[1] != 2 or flows.shape[0] == 0:
        raise ValueError(f"flows must be [B, 2, H, W] with B > 0, got shape {tuple(flows.shape)}")
    B = int(flows.shape[0])
    H, W = _image_shape(flows, "flows")
    if images.dim() == 2:
        shared = True
        images = images[None]
    elif images.dim() == 3 and int(images.shape[0]) == B:
        shared = False
    else:
        raise ValueError(f"images must be {image_dims}, got shape {tuple(images.shape)} for flows {tuple(flows.shape)}")
    if tuple(images.shape[-2:]) != (H, W):
        raise ValueError(f"images {tuple(images.shape)} and flows {tuple(flows.shape)} differ in height or width")
    if flows.dtype not in _FLOATS:
        raise ValueError(f"flows must be float32 or float64, got {flows.dtype}")
    if images.dtype != torch.uint8 and images.dtype != flows.dtype:
        raise ValueError(f"images must be uint8 or share the flows' dtype {flows.dtype}, got {images.dtype}")
    return images, flows, shared, B, H, W, flows.dtype


def warp_image_forward_batch(images, flows) -> torch.Tensor:
    """``warp_image_forward`` of B items in one launch.  images: [B, H, W], or one [H, W] image shared by all items, uint8 or of
    the flows' dtype; flows: [B, 2, H, W] float32 / float64, rows first.  Returns a device tensor [B, H, W] of the flows' dtype."""
    images, flows, shared, B, H, W, compute = _warp_inputs(images, flows, "[B, H, W] or [H, W]")
    _hip.require_gpu()
    dev = _device_of(flows, images) or default_device()
    return _warp_launch(_upload(images, dev), shared, _upload(flows, dev), None, compute, B, H, W)


def warp_image_forward(im1, forward_flow):
    """src/utils/frame_utils.py:56-89.  im1 [H, W], forward_flow [2, H, W].  numpy in: both are taken as float64 and a float64
    numpy array comes back, squeezed; tensors: the result has the flow's dtype (a float image must share it; a uint8 image goes
    with either) and stays on the flow's device."""
    _check_array(im1, "im1")
    _check_array(forward_flow, "forward_flow")
    if im1.ndim != 2 or forward_flow.ndim != 3 or tuple(forward_flow.shape) != (2,) + tuple(im1.shape):
        raise ValueError(f"im1 must be [H, W] and forward_flow [2, H, W], got shapes {tuple(im1.shape)} and {tuple(forward_flow.shape)}")
    if isinstance(im1, np.ndarray):
        if not isinstance(forward_flow, np.ndarray):
            raise ValueError("im1 is a numpy array but forward_flow is not")
        out = warp_image_forward_batch(torch.from_numpy(im1.astype(np.float64)), torch.from_numpy(forward_flow.astype(np.float64))[None])
        return out[0].cpu().numpy().squeeze()
    if not isinstance(forward_flow, torch.Tensor):
        raise ValueError("im1 is a tensor but forward_flow is not")
    return warp_image_forward_batch(im1, forward_flow[None])[0].to(forward_flow.device).squeeze()


def warp_image_torch(im1: torch.Tensor, global_shift: torch.Tensor) -> torch.Tensor:
    """src/utils/frame_utils.py:92-115.  im1 [H, W] (taken as float64, the type of the reference's grid), global_shift [2] float32 or
    float64 (rows, columns): the shift divided by (size - 1) / 2 in its own dtype is subtracted from the float32 grid in float32 (a 0-dim
    tensor does not promote the grid), and the image is sampled in float64.  Returns a
    float64 tensor [H, W] on im1's device."""
    for x, name in ((im1, "im1"), (global_shift, "global_shift")):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
        _check_array(x, name)
    if im1.dim() != 2 or tuple(global_shift.shape) != (2,):
        raise ValueError(f"im1 must be [H, W] and global_shift [2], got shapes {tuple(im1.shape)} and {tuple(global_shift.shape)}")
    if global_shift.dtype not in _FLOATS:
        raise ValueError(f"global_shift must be float32 or float64, got {global_shift.dtype}")
    H, W = _image_shape(im1, "im1")
    _hip.require_gpu()
    dev = _device_of(im1, global_shift) or default_device()
    image = _upload(im1.detach(), dev)
    if image.dtype != torch.uint8:
        image = image.double()
    out = _warp_launch(image[None], True, None, _upload(global_shift.detach(), dev).reshape(1, 2), torch.float64, 1, H, W)
    return out[0].to(im1.device).squeeze()


# ------------------------------------------------------------------------------------------------ SSIM
def _ssim_inputs(img1, img2, window_size):
    img1, img2 = _torch(_check_array(img1, "img1")), _torch(_check_array(img2, "img2"))
    ws = _window(window_size)
    if img1.dim() != 4 or tuple(img1.shape) != tuple(img2.shape) or 0 in img1.shape[:2]:
        raise ValueError(f"img1 and img2 must both be [B, C, H, W], got shapes {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.dtype != img2.dtype:
        raise ValueError(f"img1 and img2 must share a dtype, got {img1.dtype} and {img2.dtype}")
    if img1.dtype not in _FLOATS:
        raise ValueError(f"img1 and img2 must be float32 or float64, got {img1.dtype}")
    _image_shape(img1, "img1")
    return img1, img2, ws


def _ssim_launch(img1: torch.Tensor, img2: torch.Tensor, ws: int, want_means: bool):
    """-> (map [B, C, H, W], means float64 [B C + B + 1, then scratch] or None) on the device."""
    lib = _hip.require_gpu()
    if ws > max_window_size():
        raise ValueError(f"window_size {ws} > {max_window_size()} is not built")
    dev = _device_of(img1, img2) or default_device()
    a, b = _upload(img1, dev), _upload(img2, dev)
    B, C, H, W = (int(v) for v in a.shape)
    taps = window_taps(ws, a.dtype).to(dev)
    out = torch.empty_like(a)
    means = torch.empty(int(lib.ebos_ssim_means_elems(_CODES[a.dtype], B, C, H, W)), dtype=torch.float64, device=dev) if want_means else None
    fn = lib.ebos_ssim_map_f64 if a.dtype == torch.float64 else lib.ebos_ssim_map_f32
    with _hip.on_device(dev):
        check(fn(a.data_ptr(), b.data_ptr(), taps.data_ptr(), ws, B, C, H, W, out.data_ptr(), ptr(means), stream_ptr(dev)), "ebos_ssim_map")
    return out, means


def ssim_map(img1, img2, window_size=11) -> torch.Tensor:
    """The reference's SSIM map (``_ssim`` before its mean) of the image pairs img1, img2 [B, C, H, W], float32 or float64.  Returns
    a tensor [B, C, H, W] of the input dtype on the inputs' device."""
    a, b, ws = _ssim_inputs(img1, img2, window_size)
    return _ssim_launch(a, b, ws, False)[0].to(a.device)


def ssim(img1, img2, window_size=11, size_average=True) -> torch.Tensor:
    """src/utils/stat_utils.py:277-285.  img1, img2 [B, C, H, W].  ``size_average``: the mean of the whole map (0-dim); otherwise
    the mean per item, [B].  Float64 sums in a fixed order, cast to the input dtype."""
    a, b, ws = _ssim_inputs(img1, img2, window_size)
    B, C = int(a.shape[0]), int(a.shape[1])
    means = _ssim_launch(a, b, ws, True)[1]
    out = means[B * C + B] if size_average else means[B * C:B * C + B]
    return out.to(a.dtype).to(a.device)


class SSIM(torch.nn.Module):
    """src/utils/stat_utils.py:251-274: ``ssim`` with the window size and the averaging fixed at construction."""

    def __init__(self, window_size=11, size_average=True):
        super(SSIM, self).__init__()
        self.window_size = _window(window_size)
        self.size_average = size_average

    def forward(self, img1, img2):
        return ssim(img1, img2, self.window_size, self.size_average)


# ------------------------------------------------------------------------------------------------ the fused score
def _roi(roi, H: int, W: int) -> Optional[Tuple[int, int, int, int]]:
    """(xmin, xmax, ymin, ymax), rows then columns, tuple or dict -> the rectangle ``image[xmin:xmax, ymin:ymax]`` selects."""
    if roi is None:
        return None
    r = tuple(roi[k] for k in ("xmin", "xmax", "ymin", "ymax")) if isinstance(roi, dict) else tuple(roi)
    if len(r) != 4 or any(isinstance(v, bool) or int(v) != v for v in r):
        raise ValueError(f"roi must be four integers (xmin, xmax, ymin, ymax), got {roi!r}")
    x0, x1, _ = slice(int(r[0]), int(r[1])).indices(H)
    y0, y1, _ = slice(int(r[2]), int(r[3])).indices(W)
    return x0, max(x0, x1), y0, max(y0, y1)


def photometric_error_batch(frame1, frame2, flow, roi=None, mask=None, window_size=11) -> Tuple[torch.Tensor, Tuple[str, ...]]:
    """The photometric score of B items in two launches, without a host synchronisation.

    Args:
        frame1 ... [B, H, W], or one [H, W] image shared by the batch; frame2 ... [B, H, W].  uint8 or the flow's dtype, both the same.
        flow ... [B, 2, H, W] float32 / float64, rows first: the displacement from frame1 to frame2 (frame1 is sampled at x - flow).
        roi ... (xmin, xmax, ymin, ymax) or a dict of these: only rows [xmin, xmax) x columns [ymin, ymax) are counted.
        mask ... [B, H, W] or [H, W]; only pixels where it is non-zero are counted.

    Returns:
        (table, COLUMNS): a float64 device tensor [B, 7] with the columns L1, RMSE, SSIM, L1_0, RMSE_0, SSIM_0, n_points.  The SSIM
        maps are those of the whole images; every mean runs over the counted pixels.  A row with n_points = 0 is NaN otherwise.
    """
    frame2 = _torch(_check_array(frame2, "frame2"))
    f1, fl, shared, B, H, W, compute = _warp_inputs(_check_array(frame1, "frame1"), _check_array(flow, "flow"), "[B, H, W] or [H, W]")
    ws = _window(window_size)
    if tuple(frame2.shape) != (B, H, W):
        raise ValueError(f"frame2 must be [B, H, W] = {(B, H, W)}, got shape {tuple(frame2.shape)}")
    if frame2.dtype != f1.dtype:
        raise ValueError(f"frame1 and frame2 must share a dtype, got {f1.dtype} and {frame2.dtype}")
    rect = _roi(roi, H, W)
    m = None
    if mask is not None:
        m = _torch(_check_array(mask, "mask"))
        if tuple(m.shape) not in ((B, H, W), (H, W)):
            raise ValueError(f"mask must be [B, H, W] = {(B, H, W)} or [H, W], got shape {tuple(m.shape)}")
    lib = _hip.require_gpu()
    if ws > max_window_size():
        raise ValueError(f"window_size {ws} > {max_window_size()} is not built")
    dev = _device_of(fl, f1, frame2) or default_device()
    f1, f2, fl = _upload(f1, dev), _upload(frame2, dev), _upload(fl, dev)
    mask_sb = 0
    if m is not None:
        m = _upload(m, dev)
        m = m.view(torch.uint8) if m.dtype == torch.bool else (m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8))
        mask_sb = H * W if m.dim() == 3 else 0
    taps = window_taps(ws, compute).to(dev)
    out = torch.empty((B, len(COLUMNS)), dtype=torch.float64, device=dev)
    nbytes = int(lib.ebos_photometric_scratch_bytes(_CODES[compute], B, H, W))
    if nbytes == 0:
        raise ValueError(f"bad geometry: {B} items of {H} x {W}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    r4 = rect or (0, 0, 0, 0)
    with _hip.on_device(dev):
        check(lib.ebos_photometric_batch(_CODES[compute], _CODES[f1.dtype], B, H, W, f1.data_ptr(), 0 if shared else H * W, f2.data_ptr(),
                                         fl.data_ptr(), taps.data_ptr(), ws, int(rect is not None), *r4, ptr(m), mask_sb, out.data_ptr(),
                                         scratch.data_ptr(), nbytes, stream_ptr(dev)), "ebos_photometric_batch")
    return out, COLUMNS


def photometric_error(frame1, frame2, flow, roi=None, mask=None, window_size=11) -> dict:
    """``photometric_error_batch`` of one item: frame1, frame2 [H, W], flow [2, H, W], mask [H, W] -> {column: np.float64} (one
    read-back)."""
    for x, name in ((frame1, "frame1"), (frame2, "frame2"), (flow, "flow")):
        _check_array(x, name)
    if frame1.ndim != 2 or frame2.ndim != 2 or flow.ndim != 3:
        raise ValueError(f"frame1 and frame2 must be [H, W] and flow [2, H, W], got shapes {tuple(frame1.shape)}, {tuple(frame2.shape)} "
                         f"and {tuple(flow.shape)}")
    if mask is not None and _check_array(mask, "mask").ndim != 2:
        raise ValueError(f"mask must be [H, W], got shape {tuple(mask.shape)}")
    table, _ = photometric_error_batch(frame1, frame2[None], flow[None], roi=roi, mask=mask, window_size=window_size)
    row = table[0].cpu().numpy()
    return {k: np.float64(row[j]) for j, k in enumerate(COLUMNS)}


__all__ = ["COLUMNS", "SSIM", "max_window_size", "photometric_error", "photometric_error_batch", "ssim", "ssim_map", "warp_image_forward",
           "warp_image_forward_batch", "warp_image_torch", "window_taps"]
