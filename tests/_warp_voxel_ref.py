"""numpy / CPU-torch restatement of the time-aware warp (``motion_model="dense-flow-voxel"``), the yardstick of
tests/test_gpu_warp_voxel.py.  The reference documents the motion model (src/warp.py:199, 211) and ships without its branch
(:223-228), so there is nothing of its own to record; tests/test_warp_voxel.py pins this file to the reference BY COMPOSITION
(tests/golden/golden_warp_voxel.npz): the events of every bin warped by the reference's own ``warp_event_from_optical_flow`` with
that bin's flow and the whole window's reference time, scattered back to input order.

  bin     tau = (t - tmin) / (tmax - tmin) per batch row in float64 whatever the event dtype; k = min(int(tau * T), T - 1);
          tmax == tmin -> 0
  warp    the reference's torch lines (src/warp.py:245-253, 283-287, 330-337) in the events' dtype, with the gather index
          ``trunc(x) * W + trunc(y)`` extended by the bin: ``k * H * W + ...`` into the voxel's channel, flattened
  splat   ``bilinear_vote_tensor`` (src/event_image_converter.py:562-620)
  gradients by CPU autograd through the lines above
"""
import numpy as np
import torch


def as_tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def time_bins(t, T: int) -> np.ndarray:
    """t [(b,) n] (any float dtype) -> int64 [(b,) n]; the window is the last axis."""
    t = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).astype(np.float64)
    tmin, tmax = t.min(axis=-1, keepdims=True), t.max(axis=-1, keepdims=True)
    span = tmax - tmin
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = (t - tmin) / span
    k = np.minimum((np.where(span > 0, tau, 0.0) * float(T)).astype(np.int64), T - 1)
    return k


def reference_time(events: torch.Tensor, direction):
    """src/warp.py:245-262 on a tensor [(b,) n, 4]."""
    t = events[..., 2]
    tmin, tmax = torch.min(t, -1).values, torch.max(t, -1).values
    if type(direction) is float:
        per = tmax - tmin
        return tmin + per * direction
    if direction == "first":
        return tmin
    if direction == "last":
        return tmax
    return reference_time(events, {"middle": 0.5, "before": -1.0, "after": 2.0}[direction])


def calculate_dt(events: torch.Tensor, ref, normalize_t: bool) -> torch.Tensor:
    """src/warp.py:283-287."""
    dt = events[..., 2] - ref
    if normalize_t:
        period = torch.max(dt, -1).values - torch.min(dt, -1).values
        dt = dt / period[..., None]
    return dt


def warp_voxel(events, voxel, direction="first", normalize_t=False, ref=None, row_stride=None, bins=None):
    """events [(b,) n, 4], voxel [(b,) T, 2, H, W] (tensors or arrays of one dtype) -> warped tensor [b, n, 4] (the batch axis
    is kept: the ``squeeze`` of the reference is the product's business).  ``ref``: an explicit reference time.  ``bins``: the
    int64 tensor [b, n] of ``time_bins`` if the caller keeps it (tools/bench_warp_voxel.py: on the device, like a plan does)."""
    ev, vx = as_tensor(events), as_tensor(voxel)
    if ref is None:
        ref = reference_time(ev, direction)
        if ev.dim() == 3:
            ref = ref[..., None]
    dt = calculate_dt(ev, ref, normalize_t)
    if ev.dim() == 2:
        ev, vx, dt = ev[None], vx[None], dt[None]
    b, T, _, H, W = vx.shape
    k = torch.from_numpy(time_bins(ev[..., 2], T)) if bins is None else bins
    ind = k * (H * W) + ev[..., 0].long() * (W if row_stride is None else row_stride) + ev[..., 1].long()
    flat = vx.reshape(b, T, 2, H * W)
    warped = ev.clone()
    warped[..., 0] = ev[..., 0] - dt * torch.gather(flat[:, :, 0].reshape(b, -1), 1, ind)
    warped[..., 1] = ev[..., 1] - dt * torch.gather(flat[:, :, 1].reshape(b, -1), 1, ind)
    warped[..., 2] = dt
    return warped


def bilinear_vote(events: torch.Tensor, image_size, pad=(0, 0), weight=1.0) -> torch.Tensor:
    """events [n, 4] -> image [H + 2 pad_h, W + 2 pad_w] in the events' dtype (src/event_image_converter.py:562-620 with
    ``outer_padding = pad``)."""
    ph, pw = pad
    h, w = image_size[0] + 2 * ph, image_size[1] + 2 * pw
    ev = events[None]
    image = ev.new_zeros((1, h * w))
    floor_xy = torch.floor(ev[..., :2] + 1e-6)
    frac = ev[..., :2] - floor_xy
    floor_xy = floor_xy.long()
    x1, y1 = floor_xy[..., 1] + pw, floor_xy[..., 0] + ph
    inds = torch.cat([x1 + y1 * w, x1 + (y1 + 1) * w, (x1 + 1) + y1 * w, (x1 + 1) + (y1 + 1) * w], dim=-1)
    mask = torch.cat([(0 <= x1) * (x1 < w) * (0 <= y1) * (y1 < h), (0 <= x1) * (x1 < w) * (0 <= y1 + 1) * (y1 + 1 < h),
                      (0 <= x1 + 1) * (x1 + 1 < w) * (0 <= y1) * (y1 < h), (0 <= x1 + 1) * (x1 + 1 < w) * (0 <= y1 + 1) * (y1 + 1 < h)],
                     dim=-1)
    if isinstance(weight, torch.Tensor):
        weight = weight[None]
    vals = torch.cat([(1 - frac[..., 0]) * (1 - frac[..., 1]) * weight, frac[..., 0] * (1 - frac[..., 1]) * weight,
                      (1 - frac[..., 0]) * frac[..., 1] * weight, frac[..., 0] * frac[..., 1] * weight], dim=-1)
    image.scatter_add_(1, (inds * mask).long(), vals * mask)
    return image.reshape(h, w)


def iwe_voxel(events, voxel, direction="first", normalize_t=True, pad=(0, 0), weight=1.0, bins=None) -> torch.Tensor:
    """Un-batched events [n, 4] and voxel [T, 2, H, W] -> the time-aware IWE (differentiable in ``voxel`` and ``weight``)."""
    vx = as_tensor(voxel)
    warped = warp_voxel(events, vx, direction, normalize_t, bins=bins)[0]
    return bilinear_vote(warped, vx.shape[-2:], pad, weight)


def image_variance(iwe: torch.Tensor, omit_boundary: bool = False) -> torch.Tensor:
    """torch.var of the image (src/costs/image_variance.py), the outermost ring left out with ``omit_boundary``."""
    return torch.var(iwe[1:-1, 1:-1] if omit_boundary else iwe)


def gradient_magnitude(iwe: torch.Tensor, omit_boundary: bool = False) -> torch.Tensor:
    """mean(gx^2 + gy^2), Sobel 3 x 3 / 8 on the replicate-padded image (src/costs/gradient_magnitude.py, SobelTorch)."""
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=iwe.dtype, device=iwe.device) / 8.0
    p = torch.nn.functional.pad(iwe[None, None], (1, 1, 1, 1), mode="replicate")
    g0 = torch.nn.functional.conv2d(p, kx[None, None])[0, 0]
    g1 = torch.nn.functional.conv2d(p, kx.t()[None, None])[0, 0]
    if omit_boundary:
        g0, g1 = g0[1:-1, 1:-1], g1[1:-1, 1:-1]
    return torch.mean(torch.square(g0) + torch.square(g1))


COSTS = {"image_variance": image_variance, "gradient_magnitude": gradient_magnitude}
