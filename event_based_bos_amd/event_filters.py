"""The reference's event filters on the GPU (reference: src/utils/event_filters.py): the background-activity filter (BAF,
:46-97), the hot-pixel filter (HOT, :100-128) and ``EventFilter`` (:154-224), which runs CROP and the filters a config lists.

Same names and signatures as the reference, same results bit for bit (kept events, their order, the final time map), computed
by the kernels of csrc/event_filters.hip instead of per-event Python loops.  numpy input gives numpy output (a numpy
``time_map`` argument is updated in place, like the reference's); a torch tensor gives a tensor on its device.  Three edge
behaviours of the reference are not copied: an empty result is an empty [0, 4] array (the reference returns ``np.array([])``
or fails in ``np.vstack``); an event whose pixel lies outside the sensor raises ``ValueError`` (the reference wraps negative
indices); a BAF neighbourhood clipped to fewer than ``num_support_event + 1`` pixels raises ``IndexError`` only when an event
lands in such a position (the reference's ``time_array[-1 - num_support_event]``), after the kernels have run.

Raw sensor windows (``RawEventStore.load_raw`` columns) are filtered by ``filter_raw_window``: the filters' keep masks are
chained on the device (each filter skips itself when fewer than 10 events reach it, like ``EventFilter.process``) and one
compaction at the end gives the kept columns -- one host read-back per window (the kept count, with the error counters).
"""
from __future__ import annotations

import logging
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import check, ptr, stream_ptr
from ._staging import to_gpu
from .types import NUMPY_TORCH

logger = logging.getLogger(__name__)

DEFAULT_INDEX_CONVENTION = {"x": 0, "y": 1, "t": 2, "p": 3}
MIN_EVENTS = 10   # EventFilter.process: fewer events -> returned as they are, the remaining filters skipped (:184-187)
MAX_KSIZE, MAX_SUPPORT = 7, 15


def _layout(index_convention: Optional[dict]) -> int:
    ic = index_convention or DEFAULT_INDEX_CONVENTION
    ix, iy, it = int(ic["x"]), int(ic["y"]), int(ic["t"])
    if not all(0 <= v < 4 for v in (ix, iy, it)) or len({ix, iy, it}) != 3:
        raise ValueError(f"index_convention {ic}: x, y and t must be distinct columns of the [n, 4] events")
    return ix | iy << 2 | it << 4


class _Window(object):
    """A window on the device as the filter kernels read it: AoS events [n, 4] (f32 / f64) or raw sensor columns."""

    def __init__(self, events: Optional[torch.Tensor] = None, raw: Optional[Tuple[torch.Tensor, ...]] = None,
                 ticks_per_second: float = 1e6, layout: int = 0x24):
        self.events, self.raw, self.tps, self.layout = events, raw, float(ticks_per_second), layout
        if events is not None:
            if events.dim() != 2 or events.shape[1] != 4 or events.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"events must be an [n, 4] float32 / float64 array, got {tuple(events.shape)} {events.dtype}")
            self.kind = _hip.FILTER_SRC_F32 if events.dtype == torch.float32 else _hip.FILTER_SRC_F64
            self.n, self.device = int(events.shape[0]), events.device
        else:
            col, row, t, pol = raw
            self.kind = _hip.FILTER_SRC_RAW32 if t.dtype == torch.int32 else _hip.FILTER_SRC_RAW64
            self.n, self.device = int(t.shape[0]), t.device

    def source(self) -> _hip.EventSource:
        s = _hip.EventSource()
        s.kind, s.layout, s.ticks_per_second, s.n = self.kind, self.layout, self.tps, self.n
        if self.events is not None:
            s.events = ptr(self.events)
        else:
            s.col, s.row, s.t, s.pol = (ptr(v) for v in self.raw)
        return s

    def fractional(self, mask: Optional[torch.Tensor]) -> bool:
        """Any (input) event with a non-integer pixel coordinate?  Raw columns never have one."""
        if self.events is None:
            return False
        ic = [self.layout & 3, (self.layout >> 2) & 3]
        xy = self.events[:, ic]
        frac = (xy != torch.trunc(xy)).any(dim=1)
        if mask is not None:
            frac &= mask.bool()
        return bool(frac.any().item())


class _Chain(object):
    """Keep masks of successive filters over ONE window, on the device; ``compact`` ends it."""

    def __init__(self, win: _Window, image_shape, vote: str = "atomic"):
        self.lib = _hip.require_gpu()
        if vote not in ("atomic", "ordered"):
            raise ValueError(f"vote must be 'atomic' or 'ordered', got {vote!r}")
        self.vote = vote   # how the hot-pixel filter's image of fractional events is accumulated (ops.splat's routes)
        self.win, self.H, self.W = win, int(image_shape[0]), int(image_shape[1])
        self.mask: Optional[torch.Tensor] = None
        self.n_dev: Optional[torch.Tensor] = None   # events in the chain's current output (device int32); None: all win.n
        dev = win.device
        self.status = torch.zeros(2, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(int(self.lib.ebos_event_filter_scratch_bytes(win.n, self.H, self.W)), dtype=torch.uint8, device=dev)

    def _outputs(self):
        return torch.empty(self.win.n, dtype=torch.uint8, device=self.win.device), torch.empty(1, dtype=torch.int32, device=self.win.device)

    def baf(self, dt: float, ksize: int, num_support_event: int, time_map: Optional[torch.Tensor]) -> torch.Tensor:
        """One BAF over the chain's current events; returns the final time map (a new device [H, W] float64 tensor)."""
        if not (0 <= int(ksize) <= MAX_KSIZE and 0 <= int(num_support_event) <= MAX_SUPPORT):
            raise NotImplementedError(f"BAF_ksize = {ksize}, BAF_num_support_event = {num_support_event}: the GPU filter supports "
                                      f"0 <= ksize <= {MAX_KSIZE} and 0 <= num_support_event <= {MAX_SUPPORT}")
        m_out = torch.empty((self.H, self.W), dtype=torch.float64, device=self.win.device)
        if time_map is not None:
            time_map = time_map.to(device=self.win.device, dtype=torch.float64).contiguous()
            if tuple(time_map.shape) != (self.H, self.W):
                raise ValueError(f"time_map has shape {tuple(time_map.shape)}, expected {(self.H, self.W)}")
        mask, n_out = self._outputs()
        src = self.win.source()
        with _hip.on_device(self.win.device):
            check(self.lib.ebos_baf_mask(_hip.C.byref(src), self.H, self.W, ptr(self.mask), ptr(self.n_dev), float(dt), int(ksize),
                                         int(num_support_event), ptr(time_map), ptr(m_out), ptr(mask), ptr(n_out), ptr(self.status),
                                         ptr(self.scratch), self.scratch.numel(), stream_ptr()), "ebos_baf_mask")
        self.mask, self.n_dev = mask, n_out
        return m_out

    def hot(self, thresh: float) -> None:
        iwe = None
        if self.win.fractional(self.mask):
            # bilinear image of the input events (create_iwe(events, sigma=0) of the reference, the numpy eps): the float64
            # splat of the compacted input -- the mask then refers to that compacted window
            if self.mask is not None:
                self.compact_in_place()
                if self.win.n < MIN_EVENTS:
                    return
            ev = self.win.events
            if ev.dtype != torch.float64 or self.win.layout != 0x24:
                ic = [self.win.layout & 3, (self.win.layout >> 2) & 3, self.win.layout >> 4 & 3]
                ev = torch.stack([ev[:, ic[0]], ev[:, ic[1]], ev[:, ic[2]], ev[:, ic[2]]], dim=1).to(torch.float64).contiguous()
            if self.vote == "ordered":
                from . import ops

                iwe = ops.splat(ev[None, :self.win.n], (self.H, self.W), (0, 0), 1.0, _hip.SPLAT_BILINEAR, 1e-8, route="ordered")[0]
            else:
                iwe = torch.zeros((self.H, self.W), dtype=torch.float64, device=self.win.device)
                with _hip.on_device(self.win.device):
                    check(self.lib.ebos_splat_f64(ptr(ev), None, 1.0, _hip.SPLAT_BILINEAR, 1e-8, 1, self.win.n, self.H, self.W, 0, 0,
                                                  ptr(iwe), stream_ptr()), "ebos_splat_f64")
        mask, n_out = self._outputs()
        src = self.win.source()
        with _hip.on_device(self.win.device):
            check(self.lib.ebos_hot_mask(_hip.C.byref(src), self.H, self.W, ptr(self.mask), ptr(self.n_dev), float(thresh), ptr(iwe),
                                         ptr(mask), ptr(n_out), ptr(self.status), ptr(self.scratch), self.scratch.numel(),
                                         stream_ptr()), "ebos_hot_mask")
        self.mask, self.n_dev = mask, n_out

    def compact(self) -> _Window:
        """The kept events in order, in the window's format (one host read-back: the count and the error counters)."""
        win = self.win
        if self.mask is None:
            self._raise(self.status.cpu().numpy())
            return win
        n_out = torch.empty(1, dtype=torch.int32, device=win.device)
        if win.events is not None:
            out = torch.empty_like(win.events)
            cols = (None,) * 4
        else:
            out = None
            cols = tuple(torch.empty_like(c) for c in win.raw[:3]) + (torch.empty_like(win.raw[3]),)
        src = win.source()
        with _hip.on_device(win.device):
            check(self.lib.ebos_filter_compact(_hip.C.byref(src), ptr(self.mask), ptr(out), *(ptr(c) for c in cols), ptr(n_out),
                                               ptr(self.scratch), self.scratch.numel(), stream_ptr()), "ebos_filter_compact")
        facts = torch.cat([n_out, self.status]).cpu().numpy()
        self._raise(facts[1:])
        k = int(facts[0])
        if out is not None:
            return _Window(events=out[:k], ticks_per_second=win.tps, layout=win.layout)
        return _Window(raw=tuple(c[:k] for c in cols), ticks_per_second=win.tps, layout=win.layout)

    def compact_in_place(self) -> None:
        self.win = self.compact()
        self.mask, self.n_dev = None, None
        self.scratch = torch.empty(int(self.lib.ebos_event_filter_scratch_bytes(self.win.n, self.H, self.W)), dtype=torch.uint8,
                                   device=self.win.device)

    def _raise(self, status) -> None:
        if int(status[_hip.FILTER_STATUS_OUT_OF_SENSOR]):
            raise ValueError(f"{int(status[_hip.FILTER_STATUS_OUT_OF_SENSOR])} events lie outside the {self.H} x {self.W} sensor "
                             f"(int(x) must be in [0, H) and int(y) in [0, W))")
        if int(status[_hip.FILTER_STATUS_CLIPPED]):
            raise IndexError(f"{int(status[_hip.FILTER_STATUS_CLIPPED])} events have a BAF neighbourhood of fewer than "
                             f"num_support_event + 1 pixels (the reference's time_array[-1 - num_support_event])")


def _device_events(events: NUMPY_TORCH) -> torch.Tensor:
    ev = to_gpu(events) if isinstance(events, np.ndarray) else events
    if not ev.is_cuda:
        ev = to_gpu(ev)
    if ev.dim() == 1 and ev.numel() == 0:
        ev = ev.reshape(0, 4)
    return ev.contiguous()


def _like_input(ev: torch.Tensor, events: NUMPY_TORCH) -> NUMPY_TORCH:
    if isinstance(events, np.ndarray):
        return ev.cpu().numpy()
    return ev if events.is_cuda else ev.cpu()


# ------------------------------------------------------------------------------------------------ the reference's functions
def background_activity_filter(events: NUMPY_TORCH, image_shape: tuple, dt: float, ksize: int = 1, num_support_event: int = 1,
                               index_convention: Optional[dict] = None) -> NUMPY_TORCH:
    """src/utils/event_filters.py:25-43: the BAF from an empty time map."""
    filtered, _ = continuous_background_activity_filter(events, image_shape, dt, ksize, num_support_event, index_convention)
    return filtered


def continuous_background_activity_filter(events: NUMPY_TORCH, image_shape: tuple, dt: float, ksize: int = 1,
                                          num_support_event: int = 1, index_convention: Optional[dict] = None,
                                          time_map: Optional[NUMPY_TORCH] = None) -> Tuple[NUMPY_TORCH, NUMPY_TORCH]:
    """src/utils/event_filters.py:46-97 -> (kept events, final time map [H, W] float64).  A numpy ``time_map`` is updated in
    place (and returned); a tensor map is returned as a new tensor on the events' device; without one the map starts at zero
    and comes back as numpy for numpy events, as a device tensor for tensors."""
    ev = _device_events(events)
    win = _Window(events=ev, layout=_layout(index_convention))
    chain = _Chain(win, image_shape)
    m0 = None if time_map is None else (to_gpu(time_map) if isinstance(time_map, np.ndarray) else time_map)
    m = chain.baf(dt, ksize, num_support_event, m0)
    out = chain.compact().events
    if isinstance(time_map, np.ndarray):
        time_map[...] = m.cpu().numpy()
        m_ret = time_map
    elif time_map is None and isinstance(events, np.ndarray):
        m_ret = m.cpu().numpy()
    else:
        m_ret = m
    return _like_input(out, events), m_ret


def hot_pixel_filter(events: NUMPY_TORCH, image_shape: tuple, hot_pixel: int = 10, index_convention: Optional[dict] = None,
                     vote: str = "atomic") -> NUMPY_TORCH:
    """src/utils/event_filters.py:100-128: drops the events of pixels whose sigma = 0 image of events is > ``hot_pixel``.
    ``vote``: the route of that image for fractional coordinates ("atomic", or "ordered": the same image bit for bit every time)."""
    ev = _device_events(events)
    chain = _Chain(_Window(events=ev, layout=_layout(index_convention)), image_shape, vote)
    chain.hot(hot_pixel)
    return _like_input(chain.compact().events, events)


class EventFilter(object):
    """src/utils/event_filters.py:154-224.  ``filter_config`` = the ``solver.filter`` section: ``filters`` (list of "BAF" /
    "HOT", or None / absent), ``parameters`` (BAF_dt, BAF_ksize, BAF_num_support_event, BAF_continuous_update, HOT_thresh and,
    after config propagation, the CROP bounds xmin / xmax / ymin / ymax), optional ``index_convention``.  CROP is prepended
    when ``xmin`` is a parameter; an unknown filter name raises ``KeyError`` here.  The BAF time map lives on the device between
    ``process`` calls when BAF_continuous_update is true."""

    FILTER_NAMES = ("BAF", "HOT", "CROP")

    def __init__(self, image_shape, filter_config: dict):
        self.image_shape = tuple(int(v) for v in image_shape)
        self.filter_params = dict(filter_config.get("parameters") or {})
        listed = filter_config.get("filters")
        self.filters = [] if listed is None else list(listed)
        if "xmin" in self.filter_params:
            self.filters = ["CROP"] + self.filters
        self.index_convention = filter_config.get("index_convention", DEFAULT_INDEX_CONVENTION)
        self.continuous_update = bool(self.filter_params.get("BAF_continuous_update", False))
        self.vote = str(self.filter_params.get("HOT_vote", "atomic"))   # the hot-pixel image's route: "atomic" | "ordered"
        self.time_map: Optional[torch.Tensor] = None
        self.setup()

    def setup(self):
        funcs = {"BAF": self.background_activity_filter, "HOT": self.hot_pixel_filter, "CROP": self.crop}
        self.filter_func = [funcs[f] for f in self.filters]   # (KeyError for an unknown name, like the reference's FILTER_SET)
        logger.info(f"Setup filters: {self.filters} with parameters: {self.filter_params}")

    def reset(self) -> None:
        self.time_map = None

    def process(self, events: NUMPY_TORCH, skip: Sequence[str] = ()) -> NUMPY_TORCH:
        """The listed filters in order (``skip``: names left out, e.g. a CROP the caller has applied itself)."""
        ev = _device_events(events)
        names = [f for f in self.filters if f not in skip]
        k = 0
        while k < len(names):
            if ev.shape[0] < MIN_EVENTS:
                logger.warning("Too small events after filering.")
                break
            if names[k] == "CROP":
                ev = self.crop(ev)
                k += 1
                continue
            # a run of BAF / HOT: masks chained on the device, one compaction (the 10-event rule is checked by the kernels)
            run = []
            while k < len(names) and names[k] != "CROP":
                run.append(names[k])
                k += 1
            ev = self._run(_Window(events=ev, layout=_layout(self.index_convention)), run).events
        return _like_input(ev, events)

    def filter_raw_window(self, col: torch.Tensor, row: torch.Tensor, t: torch.Tensor, pol: torch.Tensor,
                          ticks_per_second: float) -> Tuple[torch.Tensor, ...]:
        """The listed BAF / HOT filters (no CROP) over one raw sensor window on the device -> the kept (col, row, t, pol)."""
        win = _Window(raw=(col.contiguous(), row.contiguous(), t.contiguous(), pol.contiguous().view(torch.uint8)),
                      ticks_per_second=ticks_per_second)
        names = [f for f in self.filters if f != "CROP"]
        if win.n < MIN_EVENTS or not names:
            return win.raw
        return self._run(win, names).raw

    def _run(self, win: _Window, names: Sequence[str]) -> _Window:
        p = self.filter_params
        chain = _Chain(win, self.image_shape, self.vote)
        for name in names:
            if name == "BAF":
                m = chain.baf(p["BAF_dt"], p["BAF_ksize"], p["BAF_num_support_event"], self.time_map)
                self.time_map = m if self.continuous_update else None
            elif name == "HOT":
                chain.hot(p["HOT_thresh"])
            if chain.win.n < MIN_EVENTS:
                break
        return chain.compact()

    # the reference's per-filter methods (:194-224)
    def crop(self, events: NUMPY_TORCH) -> NUMPY_TORCH:
        from .utils import crop_event

        p = self.filter_params
        return crop_event(events, p["xmin"], p["xmax"], p["ymin"], p["ymax"])

    def background_activity_filter(self, events: NUMPY_TORCH) -> NUMPY_TORCH:
        return self._single(events, "BAF")

    def hot_pixel_filter(self, events: NUMPY_TORCH) -> NUMPY_TORCH:
        return self._single(events, "HOT")

    def _single(self, events: NUMPY_TORCH, name: str) -> NUMPY_TORCH:
        ev = _device_events(events)
        return _like_input(self._run(_Window(events=ev, layout=_layout(self.index_convention)), [name]).events, events)
