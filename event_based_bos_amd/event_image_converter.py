"""``EventImageConverter`` -- events -> image, accumulated by hand-written gfx950 kernels.

Drop-in for the reference's ``src/event_image_converter.py`` (class ``EventImageConverter``,
:20-620 under /root/reference): same constructor, method names, defaults (incl. the differing
default ``sigma`` of ``create_iwe`` = 1 vs ``create_image_from_events_tensor`` = 0), output shapes
(``.squeeze()``) and exceptions.  numpy arrays, CPU tensors and GPU tensors are accepted; every
image is accumulated on the GPU through libebos_hip.so (``ebos_splat_*``, ``ebos_gauss1d_*``) and
returned in the caller's container type.  No CPU compute path exists.

Accumulation rule (:581-620): with eps = 1e-6 for tensors and 1e-8 for numpy arrays,
  r0 = floor(x + eps), c0 = floor(y + eps), fr = x - r0, fc = y - c0, (R, C) = (r0, c0) + padding
  img[R, C] += (1-fr)(1-fc) w;  img[R+1, C] += fr (1-fc) w;  img[R, C+1] += (1-fr) fc w;  img[R+1, C+1] += fr fc w
taps outside the padded image are dropped.

Deliberate differences (documented in DESIGN.md):
  * ``count_event_tensor`` works (the reference raises a dtype RuntimeError, :497-500) with the numpy semantics;
  * ``method="polarity"`` is also available for tensors (the reference implements it for numpy only);
  * the tensor blur needs no torchvision: 3 taps, reflect padding, as torchvision's gaussian_blur(kernel_size=3).
"""
from __future__ import annotations

import logging
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _hip, fusion, ops
from ._staging import GPU, NUMPY, back, kind_of, to_gpu
from .types import FLOAT_TORCH, NUMPY_TORCH, is_numpy, is_torch

logger = logging.getLogger(__name__)

EPS_TENSOR = 1e-6  # :586
EPS_NUMPY = 1e-8   # :528


_TAPS_ON_DEVICE: dict = {}


def _taps_on(kind: str, sigma, device: torch.device) -> torch.Tensor:
    """Blur taps resident on ``device`` (uploaded once per (kind, sigma, device): a per-call host-to-device copy
    would synchronise, and is not allowed inside a HIP-graph capture of the solver iteration)."""
    key = (kind, float(sigma), str(device))
    if key not in _TAPS_ON_DEVICE:
        taps = _scipy_gaussian_taps(sigma) if kind == "scipy" else _torchvision_taps3(sigma)
        _TAPS_ON_DEVICE[key] = taps.to(device)
    return _TAPS_ON_DEVICE[key]


def _scipy_gaussian_taps(sigma: float, truncate: float = 4.0) -> torch.Tensor:
    radius = int(truncate * float(sigma) + 0.5)
    x = torch.arange(-radius, radius + 1, dtype=torch.float64)
    k = torch.exp(-0.5 / (float(sigma) ** 2) * x ** 2)
    return k / k.sum()


def _torchvision_taps3(sigma: float) -> torch.Tensor:
    x = torch.linspace(-1.0, 1.0, 3, dtype=torch.float64)
    k = torch.exp(-0.5 * (x / float(sigma)) ** 2)
    return k / k.sum()


class EventImageConverter(object):
    """Converter of events into image representations.

    Args:
        image_size (tuple) ... (H, W)
        outer_padding (int or tuple) ... padding added on every side so that warped events that leave the
            sensor still land in the image.
        vote (str) ... "atomic" (default): float atomics on the image.  "ordered": every accumulation goes through a sorted index
            and a fixed summation order (``ops.SplatIndex``) and repeats bit for bit; the fused provenance path is the same for both.
    """

    def __init__(self, image_size: tuple, outer_padding: Union[int, Tuple[int, int]] = 0, vote: str = "atomic"):
        if vote not in ops.SPLAT_ROUTES:
            raise ValueError(f"vote must be one of {ops.SPLAT_ROUTES}, got {vote!r}")
        self.vote = vote
        if isinstance(outer_padding, (int, float)):
            self.outer_padding = (int(outer_padding), int(outer_padding))
        else:
            self.outer_padding = outer_padding
        self.image_size = tuple(int(s + 2 * p) for s, p in zip(image_size, self.outer_padding))

    def update_property(self, image_size: Optional[tuple] = None,
                        outer_padding: Optional[Union[int, Tuple[int, int]]] = None):
        # NB: like the reference (:36-48) this adds the padding once, not twice.
        if image_size is not None:
            self.image_size = image_size
        if outer_padding is not None:
            self.outer_padding = (outer_padding, outer_padding) if isinstance(outer_padding, int) else outer_padding
        self.image_size = tuple(s + p for s, p in zip(self.image_size, self.outer_padding))

    # ------------------------------------------------------------------ core accumulation
    def _accumulate(self, events, weight, mode: int, eps: float, out_dtype: Optional[torch.dtype], index=None) -> torch.Tensor:
        """-> GPU tensor [b, h, w] ([1, 2, h, w] for polarity).  ``index``: the ``ops.SplatIndex`` of these events (ordered vote)."""
        ev = to_gpu(events, dtype=out_dtype)
        if ev.dim() == 2:
            ev = ev[None]
        wt = weight
        if is_numpy(weight) or is_torch(weight):
            wt = to_gpu(weight, device=ev.device, dtype=ev.dtype)
            if wt.dim() == 0:
                pass
            elif mode == _hip.SPLAT_POLARITY:
                wt = wt.reshape(1, -1)
            else:
                wt = wt.reshape(ev.shape[0], ev.shape[1])
        if mode == _hip.SPLAT_POLARITY:
            # boolean-mask indexing in the reference flattens the batch axis (:356-362)
            ev = ev.reshape(1, -1, 4)
        if index is not None:
            return index.vote(wt, mode)
        return ops.splat(ev, self.image_size, self.outer_padding, wt, mode, eps, route=self.vote)

    def _index_of(self, ev: torch.Tensor, eps: float):
        """One index for several bilinear votes of the same events (ordered vote), else None."""
        if self.vote != "ordered":
            return None
        return ops.SplatIndex.build(ev if ev.dim() == 3 else ev[None], self.image_size, self.outer_padding, eps)

    def _finish(self, img: torch.Tensor, kind: str):
        return back(img.squeeze(), kind)

    # ------------------------------------------------------------------ public accumulators
    def bilinear_vote_numpy(self, events: np.ndarray, weight: Union[float, np.ndarray] = 1.0):
        """[(b,) n, 4] -> float64 [(b,) H, W] (numpy semantics: eps = 1e-8).  :503-560"""
        if type(weight) == np.ndarray:
            assert weight.shape == events.shape[:-1]
        img = self._accumulate(events, weight, _hip.SPLAT_BILINEAR, EPS_NUMPY, torch.float64)
        return self._finish(img, kind_of(events))

    def bilinear_vote_tensor(self, events: torch.Tensor, weight: FLOAT_TORCH = 1.0):
        """[(b,) n, 4] -> [(b,) H, W] in the events' dtype (eps = 1e-6); differentiable w.r.t. the warped
        coordinates and ``weight``.  :562-620"""
        if type(weight) == torch.Tensor:
            assert weight.shape == events.shape[:-1]
        fused = self._try_fused(events, weight)
        if fused is not None:
            return fusion.squeezed(fused)
        img = self._accumulate(events, weight, _hip.SPLAT_BILINEAR, EPS_TENSOR, None)
        return self._finish(img, kind_of(events))

    def _try_fused(self, events, weight):
        """Warped events that still carry their provenance (fusion.py) and unit weight: fused warp + IWE."""
        if not (is_torch(events) and type(weight) in (float, int) and float(weight) == 1.0):
            return None
        return fusion.fused_iwe(events, self.image_size, self.outer_padding)

    def count_event_numpy(self, events: np.ndarray):
        """+1 on each in-bounds neighbour of every event (no bilinear weights).  :407-453"""
        img = self._accumulate(events, 1.0, _hip.SPLAT_COUNT, EPS_NUMPY, torch.float64)
        return self._finish(img, kind_of(events))

    def count_event_tensor(self, events: torch.Tensor):
        """Tensor version of ``count_event_numpy`` (eps = 1e-6).  :455-501"""
        img = self._accumulate(events, 1.0, _hip.SPLAT_COUNT, EPS_TENSOR, None)
        return self._finish(img, kind_of(events))

    def _polarity(self, events, weight, eps, dtype):
        img = self._accumulate(events, weight, _hip.SPLAT_POLARITY, eps, dtype)  # [1, 2, h, w]
        return img[0]

    # ------------------------------------------------------------------ image creation (:332-405)
    def create_image_from_events_numpy(self, events: np.ndarray, method: str = "bilinear_vote",
                                       weight: Union[float, np.ndarray] = 1.0, sigma: int = 1) -> np.ndarray:
        if method == "count":
            img = self._accumulate(events, 1.0, _hip.SPLAT_COUNT, EPS_NUMPY, torch.float64).squeeze()
        elif method == "bilinear_vote":
            if type(weight) == np.ndarray:
                assert weight.shape == events.shape[:-1]
            img = self._accumulate(events, weight, _hip.SPLAT_BILINEAR, EPS_NUMPY, torch.float64).squeeze()
        elif method == "polarity":
            img = self._polarity(events, weight, EPS_NUMPY, torch.float64)
        else:
            e = f"{method = } is not supported."
            logger.error(e)
            raise NotImplementedError(e)
        if sigma > 0:
            img = self._gaussian_filter(img, sigma)
        return back(img, kind_of(events))

    def create_image_from_events_tensor(self, events: torch.Tensor, method: str = "bilinear_vote",
                                        weight: FLOAT_TORCH = 1.0, sigma: int = 0) -> torch.Tensor:
        if method == "count":
            img = self._accumulate(events, 1.0, _hip.SPLAT_COUNT, EPS_TENSOR, None).squeeze()
        elif method == "bilinear_vote":
            if type(weight) == torch.Tensor:
                assert weight.shape == events.shape[:-1]
            img = self._try_fused(events, weight)
            if img is None:
                img = self._accumulate(events, weight, _hip.SPLAT_BILINEAR, EPS_TENSOR, None).squeeze()
            else:
                img = fusion.squeezed(img)
        elif method == "polarity":
            img = self._polarity(events, weight, EPS_TENSOR, None)
        else:
            e = f"{method = } is not implemented"
            logger.error(e)
            raise NotImplementedError(e)
        if sigma > 0:
            if img.dim() == 2:
                img = img[None, None, ...]
            elif img.dim() == 3:
                img = img[:, None, ...]
            img = self._gaussian_blur3(img, sigma)
        return back(fusion.squeezed(img), kind_of(events))

    def create_iwe(self, events: NUMPY_TORCH, method: str = "bilinear_vote", sigma: int = 1) -> NUMPY_TORCH:
        """Image of warped events [(b,) H, W].  :51-73"""
        if type(events) is fusion.LazyWarped and method == "bilinear_vote" and sigma == 0:
            # the idiom's second step on warped events nobody has read: the deferred image, straight away
            img = fusion.lazy_iwe_of(events, self.image_size, self.outer_padding)
            if img is not None:
                return img
        if is_numpy(events):
            return self.create_image_from_events_numpy(events, method, sigma=sigma)
        if is_torch(events):
            return self.create_image_from_events_tensor(events, method, sigma=sigma)
        e = f"Non-supported type of events. {type(events)}"
        logger.error(e)
        raise RuntimeError(e)

    def create_eventmask(self, events: NUMPY_TORCH) -> NUMPY_TORCH:
        """Boolean [(b,) 1, H, W]: pixels touched by at least one event.  :288-301"""
        if is_numpy(events):
            return (0 != self.create_image_from_events_numpy(events, sigma=0))[..., None, :, :]
        if is_torch(events):
            return (0 != self.create_image_from_events_tensor(events, sigma=0))[..., None, :, :]
        raise RuntimeError

    # ------------------------------------------------------------------ derived images (:75-286)
    def _averaged(self, events, values, base, sigma):
        """(weighted splat) / (count splat + 1e-2) + base, optional blur -- the common shape of
        create_iwa / create_iwd / create_iwt."""
        if is_numpy(events):
            assert is_numpy(values)
            ev = to_gpu(events, dtype=torch.float64)
            val = to_gpu(values, device=ev.device, dtype=torch.float64)
            index = self._index_of(ev, EPS_NUMPY)
            num = self._accumulate(ev, val - base, _hip.SPLAT_BILINEAR, EPS_NUMPY, torch.float64, index).squeeze()
            den = self._accumulate(ev, 1.0, _hip.SPLAT_BILINEAR, EPS_NUMPY, torch.float64, index).squeeze()
            out = num / (den + 1e-2) + base
            if sigma > 0:
                out = self._gaussian_filter(out, sigma)
            return back(out, NUMPY)
        if is_torch(events):
            assert is_torch(values)
            kind = kind_of(events)
            ev = to_gpu(events)
            val = to_gpu(values, device=ev.device, dtype=ev.dtype)
            index = self._index_of(ev, EPS_TENSOR)
            num = self._accumulate(ev, val - base, _hip.SPLAT_BILINEAR, EPS_TENSOR, None, index).squeeze()
            den = self._accumulate(ev, 1.0, _hip.SPLAT_BILINEAR, EPS_TENSOR, None, index).squeeze()
            out = torch.divide(num, den + 1e-2) + base
            if out.dim() == 2:
                out = out[None, None, ...]
            elif out.dim() == 3:
                out = out[:, None, ...]
            if sigma > 0:
                out = self._gaussian_blur3(out, sigma)
            return back(out, kind)
        raise RuntimeError

    def create_iwa(self, events: NUMPY_TORCH, det_j: NUMPY_TORCH, sigma: int = 1) -> NUMPY_TORCH:
        """Image of warped area (deformation map), base 1.  :75-132"""
        return self._averaged(events, det_j, 1, sigma)

    def create_iwd(self, events: NUMPY_TORCH, div: NUMPY_TORCH, sigma: int = 1) -> NUMPY_TORCH:
        """Image of average divergence, base 0.  :134-182"""
        return self._averaged(events, div, 0, sigma)

    def create_iwt(self, events: NUMPY_TORCH, trace: NUMPY_TORCH, sigma: int = 1) -> NUMPY_TORCH:
        """Image of average trace, base 2.  :184-234"""
        return self._averaged(events, trace, 2, sigma)

    def create_iat(self, events, ts, sigma):
        pass  # empty in the reference too (:236-237)

    def create_probability_iwe(self, events: NUMPY_TORCH, prob: NUMPY_TORCH, sigma: int = 1) -> NUMPY_TORCH:
        """IWE weighted by an event-association probability.  :239-262"""
        if is_numpy(events):
            return self.create_image_from_events_numpy(events, weight=prob, sigma=sigma)
        if is_torch(events):
            return self.create_image_from_events_tensor(events, weight=prob, sigma=sigma)
        e = f"Non-supported type of events. {type(events)}"
        logger.error(e)
        raise RuntimeError(e)

    def create_timeimage(self, events: NUMPY_TORCH, ts: NUMPY_TORCH, sigma: int = 1) -> NUMPY_TORCH:
        """Sum of timestamps per pixel.  :264-286"""
        if is_numpy(events):
            assert is_numpy(ts)
            return self.create_image_from_events_numpy(events, weight=ts, sigma=sigma)
        if is_torch(events):
            assert is_torch(ts)
            return self.create_image_from_events_tensor(events, weight=ts, sigma=sigma)
        raise RuntimeError

    def create_eventrate(self, events: NUMPY_TORCH, stat: str = "max") -> NUMPY_TORCH:
        """Per-pixel maximum event rate: max over consecutive events of one pixel (in input order) of 1 / dt for
        dt > 0 (:304-327; numpy input only, like the reference).  A cold visualisation helper outside the accelerated
        path: the reference's per-event Python loop becomes a stable sort by pixel + a segmented maximum, as plain
        tensor operations on the GPU."""
        if not is_numpy(events):
            raise RuntimeError
        h, w = self.image_size
        rate = torch.zeros(h * w, dtype=torch.float64, device=to_gpu(np.zeros(1)).device)
        if stat != "max" or len(events) == 0:
            return rate.reshape(h, w).cpu().numpy()
        ev = to_gpu(events, dtype=torch.float64)
        pix = ev[:, 0].long() * w + ev[:, 1].long()  # int() truncation of the reference; raises IndexError like it
        if int(pix.min()) < 0 or int(pix.max()) >= h * w:
            raise IndexError("event outside the image in create_eventrate")
        order = torch.sort(pix, stable=True).indices
        ps, ts = pix[order], ev[order, 2]
        dt = ts[1:] - ts[:-1]
        ok = (ps[1:] == ps[:-1]) & (dt > 0)
        rate.scatter_reduce_(0, ps[1:][ok], 1.0 / dt[ok], reduce="amax", include_self=True)
        return rate.reshape(h, w).cpu().numpy()

    # ------------------------------------------------------------------ blur (K11)
    @staticmethod
    def _gaussian_filter(img: torch.Tensor, sigma) -> torch.Tensor:
        """scipy.ndimage.gaussian_filter(img, sigma) semantics: every axis, 'reflect', truncate 4 (:368-369)."""
        taps = _taps_on("scipy", sigma, img.device)
        for axis in range(img.dim()):
            img = ops.gauss1d(img, axis, taps, _hip.GAUSS_REFLECT_SCIPY)
        return img

    @staticmethod
    def _gaussian_blur3(img: torch.Tensor, sigma) -> torch.Tensor:
        """torchvision gaussian_blur(img, kernel_size=3, sigma) semantics on the last two axes (:399-404)."""
        taps = _taps_on("torch3", sigma, img.device)
        img = ops.gauss1d(img, -2, taps, _hip.GAUSS_REFLECT_TORCH)
        return ops.gauss1d(img, -1, taps, _hip.GAUSS_REFLECT_TORCH)
