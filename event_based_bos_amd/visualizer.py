"""The reference visualizer's pictures on the GPU (reference: src/visualizer.py; kernels: csrc/visualize.hip).

``Visualizer`` offers the reference's picture methods under its names and arguments -- the colour-coded flow, the flow where events
exist, the shared-scale prediction / reference pair, the Poisson-integrated density picture, the event picture -- and
``render_step_batch`` renders the ten pictures the reference driver draws per step (bos_event.py:202-207) for B windows with one
mask-close launch, one reduce launch and ten render launches, whatever B is.

    viz = Visualizer((720, 1280), save=True, save_dir="out")
    solv = solver.collections[name]((720, 1280), (720, 640), None, config["solver"], visualize_module=viz)
    solv.visualize_flows(pred, gt)          # out/flow_comparison_pred0.png, out/flow_comparison_gt0.png, out/color_wheel.png

Inputs may be numpy arrays, CPU tensors or device tensors; a rendering method returns the uint8 picture as an array of the input's
kind (the reference returns a ``PIL.Image``).  A ``PIL.Image`` is made only to write a PNG: PIL is imported when ``save=True``
(``ImportError`` from the constructor when it is absent) and nowhere else.  ``show=True`` is refused.

Deliberate differences from the reference:
  - every picture is computed in float64 whatever the input's dtype (the reference computes a float32 flow's picture in float32);
  - an all-zero flow gives a black picture and an all-zero Poisson field a picture of 128 (the reference divides 0 by 0 and casts
    NaN, which defines nothing);
  - a NaN flow component gives hue 0 (numpy's cast of a NaN angle to uint8 is undefined; 0 is what x86 produces); NaN and +-inf
    components count as 0 in the magnitude, as in the reference;
  - the 8-bit HSV -> RGB conversion and the cross-shaped mask close restate OpenCV's algorithms (tests/_viz_ref.py) and are not
    checked against OpenCV; device atan2 / sqrt can differ from libm in the last bit, so a pixel whose angle or value lies within
    rounding of an integer can differ by one hue or value step;
  - not ported: videos (``visualize_sequential_images_as_video``, ``concat_videos``), matplotlib figures, the colour branch of
    ``visualize_event`` and ``visualize_overlay_optical_flow_on_event``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, Optional, Sequence

import numpy as np
import torch

from . import _hip, event_image_converter
from ._hip import check, stream_ptr
from ._staging import NUMPY, back, default_device, kind_of

PICTURES = ("original", "original_filter", "flow_comparison_pred", "flow_comparison_gt", "pred_flow", "pred_flow_poisson",
            "pred_masked", "gt_flow", "gt_flow_poisson", "gt_masked")


# ------------------------------------------------------------------------------------------------ staging
def _device_of(*arrays) -> torch.device:
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return default_device()


def _f64(x, device: torch.device) -> torch.Tensor:
    """-> contiguous float64 device tensor."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif not isinstance(x, torch.Tensor):
        raise ValueError(f"expected a numpy array or a torch tensor, got {type(x).__name__}")
    return x.to(device=device, dtype=torch.float64).contiguous()


def _u8(x, device: torch.device) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype == torch.bool:
        x = x.to(torch.uint8)
    elif x.dtype != torch.uint8:
        x = (x != 0).to(torch.uint8)
    return x.to(device).contiguous()


def _flow4(flow, device: torch.device) -> torch.Tensor:
    f = _f64(flow, device)
    if f.dim() == 3:
        f = f[None]
    if f.dim() != 4 or f.shape[1] != 2 or f.shape[0] == 0:
        raise ValueError(f"a flow must be [B, 2, H, W] or [2, H, W], got shape {tuple(f.shape)}")
    return f


# ------------------------------------------------------------------------------------------------ the launches
def _flow_field(flow: torch.Tensor, mask: Optional[torch.Tensor] = None, pair: Optional[torch.Tensor] = None) -> dict:
    return {"kind": _hip.VIZ_FLOW if pair is None else _hip.VIZ_FLOW_PAIR, "flow": flow, "pair": pair, "mask": mask}


def _scalar_field(a: torch.Tensor) -> dict:
    return {"kind": _hip.VIZ_SCALAR, "flow": a, "pair": None, "mask": None}


def reduce_scales(fields: Sequence[dict], ord: float = 0.5) -> torch.Tensor:
    """``ebos_viz_reduce_f64``: the scalar each field's picture is normalised by -> float64 device tensor [B, len(fields)].

    fields ... ``_flow_field(flow [B, 2, H, W], mask [B, H, W] uint8 | None, pair [B, 2, H, W] | None)`` or
    ``_scalar_field(a [B, H, W])``: contiguous float64 device tensors of one B, H, W.  One launch for all of them."""
    lib = _hip.require_gpu()
    if not 1 <= len(fields) <= _hip.VIZ_MAX_FIELDS:
        raise ValueError(f"{len(fields)} fields (1 .. {_hip.VIZ_MAX_FIELDS})")
    first = fields[0]["flow"]
    B, H, W, dev = int(first.shape[0]), int(first.shape[-2]), int(first.shape[-1]), first.device
    table = (_hip.VizField * len(fields))()
    for k, f in enumerate(fields):
        a = f["flow"]
        if (int(a.shape[0]), int(a.shape[-2]), int(a.shape[-1])) != (B, H, W) or a.dtype != torch.float64 or not a.is_contiguous():
            raise ValueError("the fields of one reduction must be contiguous float64 tensors of one B, H, W")
        t = table[k]
        t.kind, t.x, t.sb = f["kind"], a.data_ptr(), a.stride(0)
        if f["kind"] != _hip.VIZ_SCALAR:
            t.y = a.data_ptr() + 8 * a.stride(1)
        if f["pair"] is not None:
            p = f["pair"]
            if tuple(p.shape) != tuple(a.shape) or p.dtype != torch.float64 or not p.is_contiguous():
                raise ValueError("the second flow of a pair must match the first")
            t.x2, t.y2, t.sb2 = p.data_ptr(), p.data_ptr() + 8 * p.stride(1), p.stride(0)
        if f["mask"] is not None:
            m = f["mask"]
            if tuple(m.shape) != (B, H, W) or m.dtype != torch.uint8 or not m.is_contiguous():
                raise ValueError(f"a mask must be a contiguous uint8 [B, H, W] = {(B, H, W)} tensor")
            t.mask, t.mask_sb = m.data_ptr(), m.stride(0)
    out = torch.empty((B, len(fields)), dtype=torch.float64, device=dev)
    with _hip.on_device(dev):
        check(lib.ebos_viz_reduce_f64(B, H, W, C.addressof(table), len(fields), float(ord), out.data_ptr(), stream_ptr(dev)),
              "ebos_viz_reduce_f64")
    return out


def flow_rgb(flow: torch.Tensor, scale: torch.Tensor, mask: Optional[torch.Tensor] = None, mask_mode: int = 0,
             ord: float = 0.5) -> torch.Tensor:
    """``ebos_viz_flow_rgb_u8``: flow [B, 2, H, W] contiguous float64, scale a float64 device view with one element per window
    (``scales[:, k]``), mask [B, H, W] uint8 -> uint8 [B, H, W, 3]."""
    lib = _hip.require_gpu()
    B, _, H, W = (int(v) for v in flow.shape)
    dev = flow.device
    if scale.dtype != torch.float64 or scale.dim() != 1 or scale.shape[0] != B or scale.device != dev:
        raise ValueError("scale must be a float64 device vector with one element per window")
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    with _hip.on_device(dev):
        check(lib.ebos_viz_flow_rgb_u8(B, H, W, flow.data_ptr(), flow.data_ptr() + 8 * flow.stride(1), flow.stride(0), scale.data_ptr(),
                                       scale.stride(0) if B > 1 else 0, None if mask is None else mask.data_ptr(),
                                       0 if mask is None else mask.stride(0), int(mask_mode) if mask is not None else 0, float(ord),
                                       out.data_ptr(), stream_ptr(dev)), "ebos_viz_flow_rgb_u8")
    return out


def hsv_to_rgb(hsv) -> Any:
    """``cv2.cvtColor(hsv, cv2.COLOR_HSV2RGB)`` on uint8 [..., 3] (hue 0 - 180) as csrc/visualize.hip restates it."""
    lib = _hip.require_gpu()
    kind = kind_of(hsv)
    dev = _device_of(hsv)
    t = torch.from_numpy(np.ascontiguousarray(hsv)) if isinstance(hsv, np.ndarray) else hsv
    if t.dtype != torch.uint8 or t.shape[-1] != 3 or t.numel() == 0:
        raise ValueError(f"hsv must be a non-empty uint8 [..., 3] array, got {t.dtype} {tuple(t.shape)}")
    t = t.to(dev).contiguous()
    out = torch.empty_like(t)
    with _hip.on_device(dev):
        check(lib.ebos_viz_hsv2rgb_u8(t.numel() // 3, t.data_ptr(), out.data_ptr(), stream_ptr(dev)), "ebos_viz_hsv2rgb_u8")
    return back(out, kind)


def mask_close(mask) -> Any:
    """``cv2.morphologyEx(mask, cv2.MORPH_CLOSE, 3 x 3 MORPH_CROSS)`` of boolean masks [B, H, W] or [H, W] -> uint8 0 / 1 of the
    same shape and kind."""
    lib = _hip.require_gpu()
    kind = kind_of(mask)
    m = _u8(mask, _device_of(mask))
    shape = tuple(m.shape)
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3 or m.numel() == 0:
        raise ValueError(f"mask must be [B, H, W] or [H, W], got shape {shape}")
    B, H, W = (int(v) for v in m.shape)
    out = torch.empty_like(m)
    with _hip.on_device(m.device):
        check(lib.ebos_viz_mask_close_u8(B, H, W, m.data_ptr(), m.stride(0), out.data_ptr(), stream_ptr(m.device)),
              "ebos_viz_mask_close_u8")
    return back(out.reshape(shape), kind)


def _gray(mode: int, a: torch.Tensor, b: Optional[torch.Tensor] = None, pad: int = 0, level: float = 0.0,
          scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``ebos_viz_gray_u8``: a, b [B, H, W] float64 device views with contiguous H x W planes -> uint8 [B, H - 2 pad, W - 2 pad]."""
    lib = _hip.require_gpu()
    B, H, W = (int(v) for v in a.shape)
    pad = int(pad)
    if pad < 0 or 2 * pad >= min(H, W):
        raise ValueError(f"padding {pad} leaves nothing of {H} x {W}")
    for t in (a, b):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (B, H, W) or t.stride(2) != 1 or t.stride(1) != W):
            raise ValueError("the planes must be float64 [B, H, W] with contiguous H x W planes")
    dev = a.device
    out = torch.empty((B, H - 2 * pad, W - 2 * pad), dtype=torch.uint8, device=dev)
    with _hip.on_device(dev):
        check(lib.ebos_viz_gray_u8(mode, B, H, W, pad, a.data_ptr(), a.stride(0), None if b is None else b.data_ptr(),
                                   0 if b is None else b.stride(0), float(level), None if scale is None else scale.data_ptr(),
                                   0 if scale is None or B == 1 else scale.stride(0), out.data_ptr(), stream_ptr(dev)),
              "ebos_viz_gray_u8")
    return out


def event_picture(counts: torch.Tensor, background_color: float = 127) -> torch.Tensor:
    """``visualize_event(grayscale=True)`` from counts [B, 2, H, W] (events per pixel with positive / negative polarity, the
    polarity image ``window_ingest_raw_batch`` leaves) -> uint8 [B, H, W]: clip(20 (n+ - n-) + background_color, 0, 255)."""
    return _gray(_hip.VIZ_GRAY_EVENT, counts[:, 0], counts[:, 1], 0, background_color)


def clipped_iwe_picture(iwe: torch.Tensor, max_scale: float = 50, pad: int = 0, second: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``create_clipped_image``: 255 - uint8(clip(max_scale iwe, 0, 255)) of iwe [B, H, W] (+ ``second``, e.g. the two polarity
    counts), then the ``outer_padding`` crop -> uint8 [B, H - 2 pad, W - 2 pad]."""
    return _gray(_hip.VIZ_GRAY_IWE, iwe, second, pad, max_scale)


def centered_picture(a: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``standardize_image_center(a).astype(uint8)`` of a [B, H, W] with scale = max |a| per window (``reduce_scales``)."""
    return _gray(_hip.VIZ_GRAY_CENTER, a, None, 0, 0.0, scale)


_WHEELS: dict = {}


def color_wheel(H: int, device: Optional[torch.device] = None) -> torch.Tensor:
    """The [H, H, 3] colour wheel of ``color_optical_flow``: the colour kernel on a ``linspace(-1, 1, H)`` meshgrid at ord 1.
    Rendered once per (H, device)."""
    device = device or default_device()
    key = (int(H), str(device))
    if key not in _WHEELS:
        xx, yy = np.meshgrid(np.linspace(-1, 1, int(H)), np.linspace(-1, 1, int(H)))
        grid = _f64(np.stack([xx, yy])[None], device)
        _WHEELS[key] = flow_rgb(grid, reduce_scales([_flow_field(grid)], 1.0)[:, 0], ord=1.0)[0]
    return _WHEELS[key]


# ------------------------------------------------------------------------------------------------ a driver step, batched
def render_step_batch(pred_flow, gt_flow, event_mask, filter_counts, orig_counts, outer_padding: int = 0, max_scale: float = 50,
                      ord: float = 0.5, return_poisson: bool = False) -> Dict[str, torch.Tensor]:
    """The ten pictures the reference driver draws per step (bos_event.py:202-207), for B windows at once.

    Args:
        pred_flow ... [B, 2, H, W]: the estimate already scaled by ``gt_time_scale / batch_time_scale``.
        gt_flow ... [B, 2, H, W]: the reference (frame-based) flow.
        event_mask ... [B, H, W] bool / uint8: pixels with a filtered event (``create_eventmask``, or ``PreparedWindows.mask``).
        filter_counts ... [B, 2, H, W]: the filtered events per pixel with positive / negative polarity (``PreparedWindows.pol``).
        orig_counts ... [B, 2, H, W]: the same for the unfiltered events between the two frames.
        outer_padding, max_scale ... the solver's ``outer_padding`` and ``max_scale`` (the clipped IWE).
    Returns:
        {name: uint8 device tensor [B, ...]} for ``PICTURES`` ([B, H, W, 3] colour, [B, H, W] grey; ``original_filter`` is
        [B, H - 2 pad, W - 2 pad]); with ``return_poisson`` also "poisson_pred" / "poisson_gt", the float64 fields.
    Launches: one mask close, the Poisson integration of both flows in one batch, one reduce and ten render launches.  A window's
    pictures have the same bits alone and in a batch.  Nothing is read back."""
    from .poisson import poisson_reconstruct_batch

    dev = _device_of(pred_flow, gt_flow, event_mask, filter_counts, orig_counts)
    pred, gt = _flow4(pred_flow, dev), _flow4(gt_flow, dev)
    if pred.shape != gt.shape:
        raise ValueError(f"pred_flow {tuple(pred.shape)} and gt_flow {tuple(gt.shape)} differ")
    B, _, H, W = (int(v) for v in pred.shape)
    mask = _u8(event_mask, dev).reshape(-1, H, W)
    fc, oc = _f64(filter_counts, dev).reshape(-1, 2, H, W), _f64(orig_counts, dev).reshape(-1, 2, H, W)
    if not (mask.shape[0] == fc.shape[0] == oc.shape[0] == B):
        raise ValueError("the event inputs must hold one entry per window")
    closed = mask_close(mask)
    both = poisson_reconstruct_batch(torch.cat([pred, gt]))          # [2 B, H, W]
    p_pred, p_gt = both[:B], both[B:]
    s = reduce_scales([_flow_field(pred, pair=gt), _flow_field(pred), _flow_field(gt), _flow_field(pred, mask=closed),
                       _flow_field(gt, mask=closed), _scalar_field(p_pred), _scalar_field(p_gt)], ord)
    on_mask = _hip.VIZ_MASK_MULTIPLY | _hip.VIZ_MASK_BLACK
    out = {
        "original": event_picture(oc),
        "original_filter": clipped_iwe_picture(fc[:, 0], max_scale, outer_padding, second=fc[:, 1]),
        "flow_comparison_pred": flow_rgb(pred, s[:, 0], ord=ord),
        "flow_comparison_gt": flow_rgb(gt, s[:, 0], ord=ord),
        "pred_flow": flow_rgb(pred, s[:, 1], ord=ord),
        "pred_flow_poisson": centered_picture(p_pred, s[:, 5]),
        "pred_masked": flow_rgb(pred, s[:, 3], closed, on_mask, ord),
        "gt_flow": flow_rgb(gt, s[:, 2], ord=ord),
        "gt_flow_poisson": centered_picture(p_gt, s[:, 6]),
        "gt_masked": flow_rgb(gt, s[:, 4], closed, on_mask, ord),
    }
    if return_poisson:
        out["poisson_pred"], out["poisson_gt"] = p_pred, p_gt
    return out


# ------------------------------------------------------------------------------------------------ the reference's class
def _pil_image():
    from PIL import Image

    return Image


class Visualizer(object):
    """src/visualizer.py:25-616 for the pictures listed in the module docstring.

    Args:
        image_shape (tuple) ... (H, W); needed to draw events.
        show (bool) ... must be False: nothing is shown from a GPU job.
        save (bool) ... write every picture under ``save_dir`` as the reference names it (needs PIL).
        save_dir (str) ... default "./"; created when missing.
    """

    def __init__(self, image_shape: tuple, show=False, save=False, save_dir=None) -> None:
        if show:
            raise NotImplementedError("show=True is not supported: pictures are returned and, with save=True, written")
        if save:
            _pil_image()   # ImportError here, not at the first picture
        self.update_image_shape(image_shape)
        self._show = False
        self._save = bool(save)
        if save_dir is None:
            save_dir = "./"
        self.update_save_dir(save_dir)
        self.default_prefix = ""
        self.default_save_count = 0
        self.prefixed_save_count: Dict[str, int] = {}

    def update_image_shape(self, image_shape):
        self._image_size = image_shape
        self._image_height = image_shape[0]
        self._image_width = image_shape[1]
        self.imager = event_image_converter.EventImageConverter(image_shape)

    def update_save_dir(self, new_dir: str) -> None:
        self.save_dir = new_dir
        if not os.path.exists(self.save_dir):
            os.makedirs(self.save_dir)

    def get_filename_from_prefix(self, prefix: Optional[str] = None, file_format: str = "png") -> str:
        """``{save_dir}/{prefix}{count}.{file_format}``; the prefix's count goes up with every call (:71-97)."""
        if prefix is None or prefix == "":
            file_name = os.path.join(self.save_dir, f"{self.default_prefix}{self.default_save_count}.{file_format}")
            self.default_save_count += 1
        else:
            try:
                self.prefixed_save_count[prefix] += 1
            except KeyError:
                self.prefixed_save_count[prefix] = 0
            file_name = os.path.join(self.save_dir, f"{prefix}{self.prefixed_save_count[prefix]}.{file_format}")
        return file_name

    def rollback_save_count(self, prefix: Optional[str] = None):
        """One step back, so that a .npy and the .png after it share a number (:99-112)."""
        if prefix is None or prefix == "":
            self.default_save_count -= 1
        else:
            try:
                self.prefixed_save_count[prefix] -= 1
            except KeyError:
                raise ValueError("The visualization save count error")

    def reset_save_count(self, file_prefix: Optional[str] = None):
        if file_prefix is None or file_prefix == "":
            self.default_save_count = 0
        elif file_prefix == "all":
            self.default_save_count = 0
            self.prefixed_save_count = {}
        else:
            del self.prefixed_save_count[file_prefix]

    def _show_or_save_image(self, image: np.ndarray, file_prefix: Optional[str] = None, fixed_file_name: Optional[str] = None):
        """Write the uint8 picture (a host array) when saving is on; the only place a ``PIL.Image`` is made (:123-143)."""
        if not self._save:
            return
        im = _pil_image().fromarray(image)
        if fixed_file_name is not None:
            im.save(os.path.join(self.save_dir, f"{fixed_file_name}.png"))
        else:
            im.save(self.get_filename_from_prefix(file_prefix))

    def _emit(self, picture: torch.Tensor, kind: str, file_prefix=None, fixed_file_name=None):
        """Save the device picture if asked and hand it back in the caller's container."""
        if self._save:
            self._show_or_save_image(picture.cpu().numpy(), file_prefix, fixed_file_name)
        return back(picture, kind)

    # ------------------------------------------------------------------ images
    def visualize_image(self, image: Any, file_prefix: Optional[str] = None):
        """Save an image: a file name, a uint8 numpy array / tensor, or a PIL image -> the picture as given (:174-187)."""
        if isinstance(image, str):
            with _pil_image().open(image) as im:
                image = np.array(im)
        if isinstance(image, torch.Tensor):
            self._show_or_save_image(image.detach().cpu().numpy(), file_prefix)
        elif isinstance(image, np.ndarray):
            self._show_or_save_image(image, file_prefix)
        else:
            self._show_or_save_image(np.array(image), file_prefix)
        return image

    def create_clipped_iwe_for_visualization(self, events, max_scale=50):
        """255 - uint8(clip(max_scale IWE, 0, 255)) of the bilinear vote of ``events`` [n, 4] (:189-201)."""
        kind = kind_of(events)
        iwe = self.imager.create_image_from_events_numpy(events, method="bilinear_vote", sigma=0) if kind == NUMPY else \
            self.imager.create_image_from_events_tensor(events, method="bilinear_vote", sigma=0)
        iwe = _f64(iwe, _device_of(iwe)).reshape(1, *self.imager.image_size)
        return back(clipped_iwe_picture(iwe, max_scale)[0], kind)

    # ------------------------------------------------------------------ optical flow
    def _color(self, fx, fy, max_magnitude, ord, mask=None, mask_mode=0):
        dev = _device_of(fx, fy)
        flow = torch.stack([_f64(fx, dev), _f64(fy, dev)])[None]
        if flow.dim() != 4:
            raise ValueError(f"flow_x and flow_y must be [H, W], got {tuple(flow.shape[2:])}")
        m = None if mask is None else _u8(mask, dev).reshape(1, *flow.shape[2:])
        if max_magnitude is None:
            scale = reduce_scales([_flow_field(flow, mask=m if mask_mode & _hip.VIZ_MASK_MULTIPLY else None)], ord)[:, 0]
        else:
            scale = torch.full((1,), float(max_magnitude), dtype=torch.float64, device=dev)
        return flow_rgb(flow, scale, m, mask_mode, ord)[0], scale

    def color_optical_flow(self, flow_x, flow_y, max_magnitude=None, ord=1.0):
        """Colour-code a flow: hue = direction, value = magnitude ** ord over ``max_magnitude`` (default: the flow's own maximum)
        -> (flow_rgb [H, W, 3] uint8, color_wheel [H, H, 3] uint8, max_magnitude float) (:372-416).  An all-zero flow (maximum 0)
        is black: the reference's 0 / 0 casts a NaN to uint8, which defines nothing."""
        kind = kind_of(flow_x)
        rgb, scale = self._color(flow_x, flow_y, max_magnitude, ord)
        wheel = color_wheel(int(rgb.shape[0]), rgb.device)
        return back(rgb, kind), back(wheel, kind), float(scale.item()) if max_magnitude is None else max_magnitude

    def visualize_optical_flow(self, flow_x, flow_y, visualize_color_wheel: bool = True, file_prefix: Optional[str] = None,
                               save_flow: bool = False, ord: float = 0.5):
        """Colour picture of a flow; ``save_flow`` also writes [flow_x, flow_y] as ``{prefix}{count}.npy`` under the number of the
        picture (:205-236)."""
        kind = kind_of(flow_x)
        if save_flow:
            save_name = self.get_filename_from_prefix(file_prefix).replace("png", "npy")
            np.save(save_name, np.stack([_host(flow_x), _host(flow_y)], axis=0))
            self.rollback_save_count(file_prefix)
        rgb, _ = self._color(flow_x, flow_y, None, ord)
        image = self._emit(rgb, kind, file_prefix)
        if visualize_color_wheel:
            self._emit(color_wheel(int(rgb.shape[0]), rgb.device), kind, fixed_file_name="color_wheel")
        return image

    def visualize_optical_flow_on_event_mask(self, flow, events, file_prefix: Optional[str] = None, ord: float = 0.5,
                                             max_color_on_mask: bool = True, mask_color: str = "white", mask_morph: bool = False):
        """The flow [2, H, W] where events [n, 4] exist, the rest painted ``mask_color`` ("white", else black); ``mask_morph``
        closes the event mask with a 3 x 3 cross first; ``max_color_on_mask`` scales by the masked flow's maximum (:271-331)."""
        kind = kind_of(flow)
        mask = self.imager.create_eventmask(events)
        dev = _device_of(flow, mask)
        mask = _u8(mask, dev).reshape(1, *self.imager.image_size)
        if mask_morph:
            mask = mask_close(mask)
        mode = (_hip.VIZ_MASK_WHITE if mask_color == "white" else _hip.VIZ_MASK_BLACK) | (_hip.VIZ_MASK_MULTIPLY if max_color_on_mask else 0)
        rgb, _ = self._color(flow[0], flow[1], None, ord, mask, mode)
        return self._emit(rgb, kind, file_prefix)

    def visualize_optical_flow_pred_and_gt(self, flow_pred, flow_gt, visualize_color_wheel: bool = True,
                                           pred_file_prefix: Optional[str] = None, gt_file_prefix: Optional[str] = None,
                                           ord: float = 0.5):
        """Both flows [2, H, W] on the scale of the larger maximum (:333-370) -> (pred picture, gt picture)."""
        kind = kind_of(flow_pred)
        dev = _device_of(flow_pred, flow_gt)
        pred, gt = _flow4(flow_pred, dev), _flow4(flow_gt, dev)
        scale = reduce_scales([_flow_field(pred, pair=gt)], ord)[:, 0]
        color_pred, color_gt = flow_rgb(pred, scale, ord=ord)[0], flow_rgb(gt, scale, ord=ord)[0]
        out = (self._emit(color_pred, kind, pred_file_prefix), self._emit(color_gt, kind, gt_file_prefix))
        if visualize_color_wheel:
            self._emit(color_wheel(int(pred.shape[2]), dev), kind, fixed_file_name="color_wheel")
        return out

    # ------------------------------------------------------------------ Poisson integration
    def visualize_poisson_integration(self, flow, file_prefix: Optional[str] = None):
        """The Poisson-integrated flow [2, H, W] (zero boundary) centred on 128 (:419-434); an all-zero field is 128 everywhere."""
        from .poisson import poisson_reconstruct_batch

        kind = kind_of(flow)
        p = poisson_reconstruct_batch(_flow4(flow, _device_of(flow)))
        return self._emit(centered_picture(p, reduce_scales([_scalar_field(p)])[:, 0])[0], kind, file_prefix)

    # ------------------------------------------------------------------ events
    def visualize_event(self, events: Any, grayscale: bool = True, background_color: int = 127, ignore_polarity: bool = False,
                        file_prefix: Optional[str] = None):
        """Events [n, 4] as a grey picture: clip(20 (n+ - n-) + background_color, 0, 255), coordinates clipped into the image
        and truncated, polarity 0 / 1 or -1 / +1 (:438-488).  ``grayscale=False`` is not ported."""
        if not grayscale:
            raise NotImplementedError("the colour event picture (grayscale=False) is not ported")
        kind = kind_of(events)
        H, W = self._image_size[0], self._image_size[1]
        dev = _device_of(events)
        ev = _f64(events, dev).reshape(-1, events.shape[-1])
        x = torch.clamp(ev[:, 0], 0, H - 1).to(torch.int32).double()
        y = torch.clamp(ev[:, 1], 0, W - 1).to(torch.int32).double()
        if ignore_polarity or ev.shape[0] == 0:
            pol = torch.ones_like(x)
        else:
            pol = ev[:, 3] * 2 - 1 if float(ev[:, 3].min()) == 0 else ev[:, 3]
        if ev.shape[0]:
            # unit votes on integer pixels through the splat kernel: channel 0 counts pol > 0, channel 1 the rest
            sel = torch.stack([x, y, torch.zeros_like(x), (pol > 0).double()], dim=1)
            counts = self.imager.create_image_from_events_tensor(sel, method="polarity", sigma=0).reshape(1, 2, H, W).contiguous()
        else:
            counts = torch.zeros((1, 2, H, W), dtype=torch.float64, device=dev)
        return self._emit(event_picture(counts, background_color)[0], kind, file_prefix)

    def save_array(self, array, file_prefix: Optional[str] = None, new_prefix: bool = False) -> None:
        """``np.save`` under the naming rule of the pictures; the count is rolled back unless ``new_prefix`` (:490-511)."""
        save_name = self.get_filename_from_prefix(file_prefix).replace("png", "npy")
        np.save(save_name, _host(array))
        if not new_prefix:
            self.rollback_save_count(file_prefix)


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


__all__ = ["Visualizer", "render_step_batch", "PICTURES", "reduce_scales", "flow_rgb", "hsv_to_rgb", "mask_close", "event_picture",
           "clipped_iwe_picture", "centered_picture", "color_wheel"]
