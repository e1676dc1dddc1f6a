"""EventPlan: the device-resident, iteration-invariant form of one event window, and the fused
warp+IWE operators that run on it.

In a contrast-maximisation loop the events of a window never change -- only the
flow / motion hypothesis does.  The plan is therefore built once per window:

  AoS [n,4] (f32|f64)  --ebos_events_to_soa-->  SoA f32 (x, y, dt, p), dt evaluated in fp64
                       --ebos_bin_events---->  counting-sorted by source pixel, tile-major
                                               (+ key_offsets per source pixel, perm back to input order)

and every objective evaluation afterwards is one fused kernel over 12-16 B/event
(``iwe_dense`` / ``iwe_2dof``), its backward, and a cost kernel over the 3.7 MB image.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch.utils import _pytree

from . import _hip, ops
from ._hip import check, ptr, stream_ptr

DEFAULT_TILE = (64, 64)
DEFAULT_HALO = 32


def choose_tile(image_size: Tuple[int, int], halo: int = DEFAULT_HALO, n_cu: int = 256) -> Tuple[int, int]:
    """Tile size (among the built tile-private configurations with this halo) that fills the CUs best:
    one workgroup owns one tile, workgroups run ~one per CU, so the cost of a pass is about
    ceil(tiles / CUs) * (events of one tile + fixed per-tile work on its LDS window).
    720 x 1280 -> (45, 80): exactly 16 x 16 = 256 tiles."""
    H, W = image_size
    best, best_cost = DEFAULT_TILE, None
    for th, tw, hl in _hip.slab_configs():
        if hl != halo:
            continue
        tiles = ((H + th - 1) // th) * ((W + tw - 1) // tw)
        rounds = (tiles + n_cu - 1) // n_cu
        cost = rounds * (th * tw + 0.15 * (th + 2 * hl) * (tw + 2 * hl))
        if best_cost is None or cost < best_cost:
            best, best_cost = (th, tw), cost
    return best


def parse_direction(direction: Union[str, float]) -> Tuple[int, float]:
    """Reference-time mode of src/warp.py:245-262 -> (ebos_reftime_mode, fraction)."""
    import numpy as np

    if type(direction) is float:
        return _hip.REF_FRACTION, direction
    if direction == "first":
        return _hip.REF_FIRST, 0.0
    if direction == "middle":
        return _hip.REF_FRACTION, 0.5
    if direction == "last":
        return _hip.REF_LAST, 1.0
    if direction == "random":
        return _hip.REF_FRACTION, float(np.random.uniform(low=0.0, high=1.0))
    if direction == "before":
        return _hip.REF_FRACTION, -1.0
    if direction == "after":
        return _hip.REF_FRACTION, 2.0
    raise ValueError(f"direction argument should be first, middle, last. Or float. {direction}")


def dt_bound_for(direction: Union[str, float], normalize_t: bool) -> Optional[float]:
    """max |dt| over the events of a window as the HOST knows it without looking at the events: with normalised time
    dt = (t - t_ref) / (t_max - t_min) lies in [-f, 1 - f] for a reference time at fraction f of the window
    (src/warp.py:245-253, 283-287).  None when the time stays in seconds (the bound is then the window's length: unknown here)."""
    if not normalize_t:
        return None
    _, frac = parse_direction(direction)
    return max(abs(frac), abs(1.0 - frac))


def ref_fraction_for(direction: Union[str, float]) -> Optional[float]:
    """The fraction f of the window at which a plan's reference time lies (``parse_direction``), kept on the plan as
    ``ref_fraction``; None for ``'random'``, whose draw is not kept."""
    if type(direction) is str and direction == "random":
        return None
    return float(parse_direction(direction)[1])


def resolve_halo(plan: "EventPlan", halo) -> int:
    """The ``halo`` argument of the tile-private operators -> the integer the C ABI takes.  An int is a built halo;
    ``"auto"`` asks for run-time windows per tile (``EBOS_HALO_AUTO``: each work item sizes its LDS window from a bound on ITS
    OWN displacements, |flow| over the tile x max |dt|), bounded by the largest halo built for the plan's tile; it needs a plan
    that knows its |dt| bound (normalised time) and falls back to that largest halo otherwise."""
    if halo != "auto":
        return int(halo)
    biggest = max((hl for th, tw, hl in _hip.slab_configs() if (th, tw) == tuple(plan.tile)), default=None)
    if biggest is None:
        raise ValueError(f"no tile-private kernels are built for tile {plan.tile}")
    if plan.dt_bound is None:
        return biggest
    return int(_hip.load_library().ebos_halo_auto(biggest, float(plan.dt_bound)))


def _norm_halo(plan: "EventPlan", halo):
    """None stays None (general kernels); "auto" becomes the ABI's EBOS_HALO_AUTO code on a binned plan."""
    if halo is None or halo != "auto":
        return halo
    return resolve_halo(plan, halo) if plan.binned else None


def _max_halo(halo: int) -> int:
    """the built halo behind a (possibly EBOS_HALO_AUTO-encoded) halo argument"""
    return halo if halo >= 0 else (-halo) & 255


_N_CU = {}


def _n_cu(device: torch.device) -> int:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _N_CU:
        _N_CU[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _N_CU[idx]


# per-work-item fixed work of the accumulate kernel (LDS clear, decode, slab store ~3.5 us) in events (~0.4 ns each)
PART_FIXED_EVENTS = 8192


def part_fixed_events(n_events: int, n_tiles: int, n_cu: int) -> int:
    """The fixed work of a work item in events, as ``ebos_plan_parts``' model prices it.  Where the tiles already fill the device, an
    extra work item is an extra ROUND on some CU, and a round has a floor (set-up, LDS clear, slab store) that does not shrink with
    the window: measured best on blobs of sigma 50 - 200 px at 1280 x 720 (tools/bench_skew_solver.py; four launches per iteration)
    were 65 k events at 1 M events, 32 k at 2 M, 8 - 16 k at 5 M, 8 k at 10 M -- i.e. ~6.5e10 / n (sigma 50 px at 2 M events: 88 ->
    76 us per iteration).  Few tiles on many CUs (a small sensor) keep the constant: their parts spread over idle CUs, no second round."""
    if 2 * n_tiles <= n_cu:
        return PART_FIXED_EVENTS
    return int(min(65536, max(PART_FIXED_EVENTS, 6.5e10 / max(int(n_events), 1))))


class PlanBatchLayout(NamedTuple):
    """Where the plans of ``EventPlan.build_raw_batch`` lie in the batch's buffers (elements, not bytes)."""
    n_tiles: int
    n_keys: int
    key_stride: int                 # window w: key_offsets [n_keys + 1] at w * key_stride
    grp_stride: int                 # grp_offsets [n_tiles + 1] at w * grp_stride
    part_stride: int                # part_table [5 n_tiles + 1] at w * part_stride
    capacities: Tuple[int, ...]     # slots of cpix / cdt per window: the single build's n + 3 n_tiles + 8
    slot_offsets: Tuple[int, ...]   # [B + 1]: first slot of every window, and the slots of the batch


PLAN_BATCH_ALIGN = 64   # elements: every window's arrays start on 128 bytes (u16 pixels) / 256 bytes (int32, f32) -- the tile-private
#                         kernels read 16-byte vectors, ebos_plan_lean_batch asks for slots on a multiple of 8


def plan_batch_layout(lengths: Sequence[int], image_size: Tuple[int, int], tile: Tuple[int, int]) -> PlanBatchLayout:
    """Offsets and capacities of the windows of a batched plan build from their event counts and the tile grid (host arithmetic only:
    the lengths are known before anything runs, so nothing on the device sizes anything).  A window holds exactly what the single
    build allocates for it -- empty windows included --, rounded up to ``PLAN_BATCH_ALIGN`` elements so that the next one is aligned."""
    H, W = int(image_size[0]), int(image_size[1])
    th, tw = int(tile[0]), int(tile[1])
    if H <= 0 or W <= 0 or th <= 0 or tw <= 0:
        raise ValueError("plan_batch_layout: image and tile sizes must be positive")
    n_tiles = ((H + th - 1) // th) * ((W + tw - 1) // tw)
    n_keys = n_tiles * th * tw
    up = lambda v: (v + PLAN_BATCH_ALIGN - 1) // PLAN_BATCH_ALIGN * PLAN_BATCH_ALIGN   # noqa: E731
    caps, offs = [], [0]
    for n in lengths:
        n = int(n)
        if n < 0:
            raise ValueError("plan_batch_layout: a window cannot hold a negative number of events")
        caps.append(n + 3 * n_tiles + 8)
        offs.append(offs[-1] + up(caps[-1]))
    return PlanBatchLayout(n_tiles, n_keys, up(n_keys + 1), up(n_tiles + 1), up(5 * n_tiles + 1), tuple(caps), tuple(offs))


@dataclass
class EventPlan:
    """SoA f32 event window on one GPU (optionally binned by source tile)."""

    x: Optional[torch.Tensor]             # SoA f32 (None in a lean plan: emit="compact")
    y: Optional[torch.Tensor]
    dt: Optional[torch.Tensor]
    p: Optional[torch.Tensor]
    image_size: Tuple[int, int]           # (H, W) of the sensor / flow field
    n: int                                # events in the plan (out-of-image sources dropped when binned)
    n_input: int                          # events handed to build()
    tile: Optional[Tuple[int, int]] = None
    key_offsets: Optional[torch.Tensor] = None   # int32 [n_keys + 1]
    perm: Optional[torch.Tensor] = None          # int32 [n]: input index of each planned event
    n_dropped: int = 0
    grp_offsets: Optional[torch.Tensor] = None   # compact plan: int32 [tiles + 1] group offsets
    cpix: Optional[torch.Tensor] = None          # compact plan: int16 storage of u16 (row << 8 | col), padded groups
    cdt: Optional[torch.Tensor] = None           # compact plan: f32 dt, NaN in padding slots
    part_table: Optional[torch.Tensor] = None    # adaptive work items (ebos_plan_parts): int32 [5 tiles + 1]
    dt_bound: Optional[float] = None             # max |dt| over the events as known on the host (dt_bound_for), else None
    bins: Optional[torch.Tensor] = None          # time-aware plan: uint8 [n] time bin of each planned event (ops.time_bins)
    time_bin: Optional[int] = None               # time-aware plan: the number of bins T the bins were made for
    ref_fraction: Optional[float] = None         # the reference time of dt as a fraction of the window (None: 'random', or unknown)
    normalized_t: Optional[bool] = None          # was dt divided by the window's length?

    @property
    def binned(self) -> bool:
        return self.key_offsets is not None

    @property
    def device(self) -> torch.device:
        return (self.x if self.x is not None else self.key_offsets).device

    @property
    def lean(self) -> bool:
        """True for a plan that holds ONLY what the tile-private kernels read (compact events + offsets): no SoA arrays,
        no permutation -- per-event weights and the general (global-atomic) kernels are not available on it."""
        return self.x is None

    @property
    def compact(self) -> bool:
        """True when the tile-private kernels read the 6 B/event format (u16 pixel + f32 dt)."""
        return self.cpix is not None

    def clear_cache(self) -> None:
        """Free what the operators cached on the plan: workspaces, dense jobs and the sweep lanes of ``variance_2dof`` /
        ``variance_dense_many`` (streams, one workspace per hypothesis of a chunk, image buffers -- up to 1.7 GB at 1280x720)."""
        for k in ("_workspaces", "_jobs", "_sweep_lanes", "_multiref_dts", "_canonical_stack"):
            self.__dict__.pop(k, None)

    def resolve_splits(self, splits: Optional[int]) -> int:
        """``splits`` of the tile-private forward kernels: k >= 1 cuts every tile into k equal parts, 0 uses the plan's
        adaptive work items (heavy tiles cut into parts, ``ebos_plan_parts``).  ``None`` picks 0 when the plan has a
        split tile -- or cannot know, having been built without a host read-back -- and 1 otherwise (a plan whose tiles
        are even gains nothing from the 2x work-item grid)."""
        if splits is not None:
            return int(splits)
        if self.part_table is None:
            return 1
        used = self.__dict__.get("_parts_used")
        n_tiles = (self.part_table.numel() - 1) // 5
        return 1 if used is not None and used <= n_tiles else 0

    # The optimiser LOOPS (FusedPatchLoop / Fused2dofLoop: forward + backward + step per iteration) pay ~24 us per iteration for the
    # passes that sum the parts of the adaptive work items, and ~0.5 us per 1000 events their fullest tile holds beyond the average
    # one when every tile is ONE work item (2 M events at 1280x720, DESIGN 4.4 #62: fullest tile 2 x the average 66.9 us adaptive
    # against 48.8 with one item per tile, 6 x 70.9 against 63.4, 21 x 95 against 197): adaptive where that excess is large enough
    LOOP_ADAPTIVE_MIN_EXCESS = 48_000

    def resolve_loop_splits(self, splits: Optional[int]) -> int:
        """``resolve_splits`` for an optimiser loop: the adaptive work items only where the fullest tile holds at least
        ``LOOP_ADAPTIVE_MIN_EXCESS`` events more than the average tile."""
        s = self.resolve_splits(splits)
        fullest = self.__dict__.get("_fullest_tile")
        if splits is None and s == 0 and fullest is not None:
            n_tiles = (self.part_table.numel() - 1) // 5
            if fullest - self.n / max(n_tiles, 1) < self.LOOP_ADAPTIVE_MIN_EXCESS:
                return 1
        return s

    def _compact_ptrs(self):
        return (ptr(self.grp_offsets), ptr(self.cpix), ptr(self.cdt)) if self.compact else (None, None, None)

    @property
    def fractional(self) -> bool:
        """True when ``bin()`` found fractional source coordinates (undistorted events) and ``frac_compact`` is, or will be, the
        layout of the grid-sampling and resident kernels.  Launches nothing."""
        return bool(self.__dict__.get("_frac_pending")) or self.__dict__.get("_frac") is not None

    def _frac_ptrs(self, query: bool = False):
        """Pointers of ``frac_compact``.  ``query``: for a ``*_supported`` check, which reads whether a launch gets the arrays, never
        what they hold -- a layout not built yet stays so, named by non-NULL stand-ins."""
        if query and self.__dict__.get("_frac") is None:
            return (1,) * 5
        return tuple(ptr(t) for t in self.frac_compact)

    def record_stream(self, stream: torch.cuda.Stream) -> None:
        """Mark every device tensor of the plan -- the fraction layout once it is built -- as in use on ``stream`` (a plan built
        on one stream and read on another)."""
        for t in (*(getattr(self, f.name) for f in fields(self)), *(self.__dict__.get("_frac") or ())):
            if isinstance(t, torch.Tensor):
                t.record_stream(stream)

    @property
    def frac_compact(self):
        """(grp_offsets, cpix, cdt, cfx, cfy) of a plan whose source coordinates are fractional (undistorted events) -- the compact
        layout with the fractions per slot, read by the resident loops and the grid-sampling launches --, or None.  Built on the first
        access, on the current stream (``ebos_plan_compact_frac_f32``: every source pixel's events in a canonical order, so two builds
        of one window hold identical slots): only launches read it, yes/no questions ask ``fractional``."""
        d = self.__dict__
        if d.get("_frac") is None and d.get("_frac_pending"):
            lib = _hip.require_gpu()
            dev = self.x.device
            H, W = self.image_size
            th, tw = self.tile
            n_tiles = ((H + th - 1) // th) * ((W + tw - 1) // tw)
            cap = self.n + 3 * n_tiles + 8
            f_grp = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
            f_pix = torch.zeros(cap, dtype=torch.int16, device=dev)
            f_dt = torch.full((cap,), float("nan"), dtype=torch.float32, device=dev)
            f_x, f_y = torch.zeros(cap, dtype=torch.float32, device=dev), torch.zeros(cap, dtype=torch.float32, device=dev)
            with _hip.on_device(dev):
                check(lib.ebos_plan_compact_frac_f32(ptr(self.x), ptr(self.y), ptr(self.dt), ptr(self.key_offsets), self.n, H, W, th, tw,
                                                     ptr(f_grp), ptr(f_pix), ptr(f_dt), ptr(f_x), ptr(f_y), cap, stream_ptr()),
                      "ebos_plan_compact_frac")
            d["_frac"], d["_frac_pending"] = (f_grp, f_pix, f_dt, f_x, f_y), False
        return d.get("_frac")

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def build(events: torch.Tensor, image_size: Tuple[int, int], direction: Union[str, float] = "first",
              normalize_t: bool = True, tile: Optional[Tuple[int, int]] = DEFAULT_TILE, emit: str = "full",
              deferred: bool = False, time_bin: Optional[int] = None) -> "EventPlan":
        """events: [n, 4] (x=row, y=col, t, p), float32 or float64, on the GPU.

        ``tile=None`` keeps the input (time) order: only the general global-atomic kernels apply;
        ``tile="auto"`` picks the tile-private configuration that fills the GPU best (``choose_tile``).
        ``emit="compact"``: the LEAN build (``ebos_plan_lean``) -- only the compact events and offsets the tile-private
        kernels read, built by a two-level counting sort in a third of the time; such a plan takes no per-event weights
        (``plan.lean``).  Windows with fractional source coordinates fall back to the full build.
        ``time_bin=T``: a time-aware plan -- the time bin of every event among T bins (``ops.time_bins``: float64, the window's own
        time range) is computed once in input order and kept permuted like the events (``plan.bins``, ``plan.time_bin``) for
        ``iwe_voxel`` / ``contrast_voxel``.  Needs ``emit="full"`` and ``deferred=False``, the standing of per-event weights."""
        if emit not in ("full", "compact"):
            raise ValueError("emit must be 'full' or 'compact'")
        if time_bin is not None:
            time_bin = ops.check_time_bins(time_bin)
            if emit != "full" or deferred:
                raise NotImplementedError('EventPlan.build: time_bin needs the SoA events and the permutation of emit="full" with '
                                          "deferred=False (a lean, compact or deferred plan keeps neither)")
        if isinstance(tile, str):
            if tile != "auto":
                raise ValueError("tile must be a (tile_h, tile_w) pair, None or 'auto'")
            tile = choose_tile(image_size)
        lib = _hip.require_gpu()
        if events.dim() != 2 or events.shape[-1] != 4:
            raise ValueError(f"EventPlan.build expects un-batched events [n,4], got {tuple(events.shape)}")
        if not events.is_cuda:
            raise _hip.HipUnavailableError("EventPlan.build: events must be on the GPU")
        events = events.contiguous()
        if emit == "compact" and deferred:
            # a lean plan is valid iff no source coordinate is fractional, and a deferred build never reads that count back: only
            # the raw int16 columns (build_raw) are integers by construction
            raise ValueError("EventPlan.build: emit='compact' with deferred=True needs integer source coordinates by construction: "
                             "use build_raw (sensor columns), or deferred=False")
        if emit == "compact" and tile is not None and events.shape[0] > 0:
            lean = _build_lean(0 if events.dtype == torch.float32 else 1, events, None, image_size, direction, normalize_t, tile,
                               1.0, deferred)
            if lean is not None:
                return lean
        H, W = int(image_size[0]), int(image_size[1])
        n = events.shape[0]
        ref_mode, frac = parse_direction(direction)
        dev = events.device
        tmm = ops.time_range(events[None])
        x, y, dt, p = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
        with _hip.on_device(dev):
            fn = getattr(lib, "ebos_events_to_soa_" + _hip.suffix(events.dtype))
            check(fn(ptr(events), ptr(tmm), ref_mode, frac, int(normalize_t), n, ptr(x), ptr(y), ptr(dt), ptr(p),
                     stream_ptr()), "ebos_events_to_soa")
        plan = EventPlan(x, y, dt, p, (H, W), n, n, dt_bound=dt_bound_for(direction, normalize_t),
                         ref_fraction=ref_fraction_for(direction), normalized_t=bool(normalize_t))
        if time_bin is not None:
            plan.bins, plan.time_bin = ops.time_bins(events[None], time_bin, tmm)[0], time_bin
        if tile is not None:
            plan = plan.bin(tile)
        return plan

    @staticmethod
    def build_raw(col: torch.Tensor, row: torch.Tensor, t: torch.Tensor, pol: torch.Tensor, image_size: Tuple[int, int],
                  direction: Union[str, float] = "first", normalize_t: bool = True,
                  tile: Optional[Tuple[int, int]] = DEFAULT_TILE, ticks_per_second: float = 1e6,
                  deferred: bool = False, emit: str = "full", time_bin: Optional[int] = None) -> "EventPlan":
        """Plan of a window given as raw sensor columns on the GPU -- ``raw_events/{x, y, t, p}`` of the CCS
        recordings: col int16 (sensor x), row int16 (sensor y), t int32/int64 ticks, pol bool/uint8
        (src/data_loader/ccs.py:57-66).  Same plan, bit for bit, as ``build`` on the float64 [n, 4] array the
        reference's loader makes of the window (:289-297), without materialising that array (32 B/event) anywhere."""
        if time_bin is not None:
            raise NotImplementedError('EventPlan.build_raw: a time-aware plan (time_bin) is built from the event array: '
                                      'EventPlan.build(events, ..., emit="full", time_bin=T)')
        if isinstance(tile, str):
            if tile != "auto":
                raise ValueError("tile must be a (tile_h, tile_w) pair, None or 'auto'")
            tile = choose_tile(image_size)
        lib = _hip.require_gpu()
        n = int(t.shape[0])
        for name, v, dts in (("col", col, (torch.int16,)), ("row", row, (torch.int16,)), ("t", t, (torch.int32, torch.int64)),
                             ("pol", pol, (torch.bool, torch.uint8))):
            if v.dim() != 1 or v.shape[0] != n or v.dtype not in dts:
                raise ValueError(f"EventPlan.build_raw: {name} must be a 1-D tensor of {n} elements, dtype in {dts}; "
                                 f"got {tuple(v.shape)} {v.dtype}")
            if not v.is_cuda:
                raise _hip.HipUnavailableError(f"EventPlan.build_raw: {name} must be on the GPU")
        if n == 0:
            raise IndexError("EventPlan.build_raw: empty window")  # the loader raises IndexError too (ccs.py:262-265)
        col, row, t = col.contiguous(), row.contiguous(), t.contiguous()
        pol = pol.contiguous().view(torch.uint8)
        if emit not in ("full", "compact"):
            raise ValueError("emit must be 'full' or 'compact'")
        if emit == "compact" and tile is not None:
            lean = _build_lean(2 if t.dtype == torch.int32 else 3, None, (col, row, t), image_size, direction, normalize_t, tile,
                               float(ticks_per_second), deferred)
            if lean is not None:
                return lean
        H, W = int(image_size[0]), int(image_size[1])
        ref_mode, frac = parse_direction(direction)
        dev = t.device
        ticks = torch.empty(2, dtype=torch.int64, device=dev)
        tmm = torch.empty(2, dtype=torch.float64, device=dev)
        x, y, dt, p = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
        with _hip.on_device(dev):
            check(lib.ebos_raw_time_range(ptr(t), t.element_size(), n, float(ticks_per_second), ptr(ticks), ptr(tmm),
                                          stream_ptr()), "ebos_raw_time_range")
            check(lib.ebos_raw_events_to_soa(ptr(col), ptr(row), ptr(t), t.element_size(), ptr(pol), float(ticks_per_second),
                                             ptr(tmm), ref_mode, frac, int(normalize_t), n, ptr(x), ptr(y), ptr(dt), ptr(p),
                                             stream_ptr()), "ebos_raw_events_to_soa")
        plan = EventPlan(x, y, dt, p, (H, W), n, n, dt_bound=dt_bound_for(direction, normalize_t),
                         ref_fraction=ref_fraction_for(direction), normalized_t=bool(normalize_t))
        if tile is not None:
            plan = plan.bin(tile, deferred=deferred)  # int16 columns: integer coordinates by construction
        return plan

    @staticmethod
    def build_raw_batch(col: torch.Tensor, row: torch.Tensor, t: torch.Tensor, pol: torch.Tensor, ranges: Sequence[Tuple[int, int]],
                        image_size: Tuple[int, int], direction: Union[str, float] = "first", normalize_t: bool = True,
                        tile: Tuple[int, int] = DEFAULT_TILE, ticks_per_second: float = 1e6, deferred: bool = True) -> List["EventPlan"]:
        """The lean plans (``emit="compact"``) of several windows of one recording in one set of launches (``ebos_plan_lean_batch``,
        ``ebos_plan_parts_batch``): ``ranges`` are half-open index ranges [begin, end) into the raw columns -- they may overlap and
        come in any order.  Plan k holds what ``build_raw(col[b:e], row[b:e], t[b:e], pol[b:e], ..., emit="compact")`` holds for
        range k, bit for bit: every window has its own reference time and normalisation.  The plans' tensors are views into the
        batch's buffers (``plan_batch_layout``), which live as long as any of the plans; ``record_stream`` works as on a single plan.
        ``deferred=False``: ONE read-back for all windows fills ``n_dropped``, the work items in use and the fullest tile.
        An empty range gives a plan without events (the window-by-window route raises IndexError for it, as ``build_raw`` does).
        A tile outside the LDS sort (``ebos_plan_lean_batch`` answers EBOS_ERR_UNSUPPORTED) is built window by window instead."""
        if isinstance(tile, str):
            if tile != "auto":
                raise ValueError("tile must be a (tile_h, tile_w) pair or 'auto'")
            tile = choose_tile(image_size)
        if tile is None:
            raise ValueError("EventPlan.build_raw_batch builds binned (lean) plans: tile must be a (tile_h, tile_w) pair or 'auto'")
        lib = _hip.require_gpu()
        n_total = int(t.shape[0])
        for name, v, dts in (("col", col, (torch.int16,)), ("row", row, (torch.int16,)), ("t", t, (torch.int32, torch.int64)),
                             ("pol", pol, (torch.bool, torch.uint8))):
            if v.dim() != 1 or v.shape[0] != n_total or v.dtype not in dts:
                raise ValueError(f"EventPlan.build_raw_batch: {name} must be a 1-D tensor of {n_total} elements, dtype in {dts}; "
                                 f"got {tuple(v.shape)} {v.dtype}")
            if not v.is_cuda:
                raise _hip.HipUnavailableError(f"EventPlan.build_raw_batch: {name} must be on the GPU")
        ranges = [(int(b), int(e)) for b, e in ranges]
        for b, e in ranges:
            if not 0 <= b <= e <= n_total:
                raise IndexError(f"EventPlan.build_raw_batch: range [{b}, {e}) outside the {n_total} events")
        if not ranges:
            return []
        col, row, t = col.contiguous(), row.contiguous(), t.contiguous()
        H, W = int(image_size[0]), int(image_size[1])
        th, tw = int(tile[0]), int(tile[1])

        def one_by_one():
            return [EventPlan.build_raw(col[b:e], row[b:e], t[b:e], pol[b:e], (H, W), direction, normalize_t, (th, tw), ticks_per_second,
                                        deferred=deferred, emit="compact") for b, e in ranges]

        if th > 256 or tw > 256:
            return one_by_one()
        ref_mode, frac = parse_direction(direction)
        dev, B = t.device, len(ranges)
        lay = plan_batch_layout([e - b for b, e in ranges], (H, W), (th, tw))
        n_tiles, n_keys = lay.n_tiles, lay.n_keys
        c_ranges = (C.c_int64 * (2 * B))(*[v for r in ranges for v in r])
        c_slots = (C.c_int64 * (B + 1))(*lay.slot_offsets)
        nbytes = int(lib.ebos_plan_lean_batch_scratch_bytes(c_ranges, B, H, W, th, tw))
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        key_all = torch.empty((B, lay.key_stride), dtype=torch.int32, device=dev)
        grp_all = torch.empty((B, lay.grp_stride), dtype=torch.int32, device=dev)
        part_all = torch.empty((B, lay.part_stride), dtype=torch.int32, device=dev)
        cpix_all = torch.empty(lay.slot_offsets[-1], dtype=torch.int16, device=dev)
        cdt_all = torch.empty(lay.slot_offsets[-1], dtype=torch.float32, device=dev)
        counts_all = torch.empty((B, 2), dtype=torch.int32, device=dev)
        n_cu = _n_cu(dev)
        c_fixed = (C.c_int32 * B)(*[part_fixed_events(e - b, n_tiles, n_cu) for b, e in ranges])
        with _hip.on_device(dev):
            rc = lib.ebos_plan_lean_batch(ptr(col), ptr(row), ptr(t), int(t.dtype == torch.int64), float(ticks_per_second), n_total,
                                          c_ranges, B, ref_mode, frac, int(normalize_t), H, W, th, tw, ptr(key_all), lay.key_stride,
                                          ptr(grp_all), lay.grp_stride, ptr(cpix_all), ptr(cdt_all), c_slots, ptr(counts_all), None,
                                          ptr(scratch), nbytes, stream_ptr())
            if rc == -3:  # EBOS_ERR_UNSUPPORTED (nothing was launched): geometry outside the LDS sort
                return one_by_one()
            check(rc, "ebos_plan_lean_batch")
            check(lib.ebos_plan_parts_batch(ptr(key_all), lay.key_stride, B, H, W, th, tw, n_cu, c_fixed, ptr(part_all), lay.part_stride,
                                            stream_ptr()), "ebos_plan_parts_batch")
            facts = None
            if not deferred:  # the one host read-back of the batch: (outside the image, fractional, work items in use, fullest tile) x B
                f_dev = torch.empty((B, 4), dtype=torch.int32, device=dev)
                check(lib.ebos_plan_facts_batch(ptr(key_all), lay.key_stride, B, H, W, th, tw, ptr(counts_all), ptr(part_all),
                                                lay.part_stride, ptr(f_dev), stream_ptr()), "ebos_plan_facts_batch")
                facts = f_dev.tolist()
        plans = []
        bound = dt_bound_for(direction, normalize_t)
        for w, (b, e) in enumerate(ranges):
            n = e - b
            dropped, used, fullest = (0, None, None) if facts is None else (facts[w][0], facts[w][2], facts[w][3])
            o, cap = lay.slot_offsets[w], lay.capacities[w]
            plan = EventPlan(None, None, None, None, (H, W), n - dropped, n, (th, tw), key_all[w, :n_keys + 1], None, dropped,
                             grp_all[w, :n_tiles + 1], cpix_all[o:o + cap], cdt_all[o:o + cap], part_all[w, :5 * n_tiles + 1], bound,
                             ref_fraction=ref_fraction_for(direction), normalized_t=bool(normalize_t))
            plan.__dict__["_counts"], plan.__dict__["_deferred"], plan.__dict__["_parts_used"] = counts_all[w], bool(deferred), used
            plan.__dict__["_fullest_tile"] = fullest
            plans.append(plan)
        return plans

    @staticmethod
    def stack_time_aware(plans: Sequence["EventPlan"]) -> "TimeAwarePlanStack":
        """Several binned time-aware plans of one geometry as ONE set of streams for the batched time-aware kernels
        (``TimeAwarePlanStack``)."""
        return TimeAwarePlanStack(plans)

    @staticmethod
    def build_raw_batch_time_aware(cols: Sequence[torch.Tensor], ranges: Sequence[Tuple[int, int]], image_size: Tuple[int, int],
                                   direction: Union[str, float], tile: Tuple[int, int], time_bin: int, roi=None, remove=None,
                                   ticks_per_second: float = 1e6, normalize_t: bool = True) -> "TimeAwarePlanStack":
        """The binned time-aware plans of several windows of one recording, stacked, from the raw sensor columns in one set of
        launches: ``TimeAwarePlanStack.from_raw``."""
        return TimeAwarePlanStack.from_raw(cols, ranges, image_size, direction, tile, time_bin, roi=roi, remove=remove,
                                           ticks_per_second=ticks_per_second, normalize_t=normalize_t)

    def bin(self, tile: Tuple[int, int] = DEFAULT_TILE, deferred: bool = False) -> "EventPlan":
        """Counting-sort the plan by source pixel, tile-major (ebos_bin_events_f32).

        ``deferred=True`` skips the one host read-back of the build (how many events lie outside the image / have
        fractional coordinates), so that a whole window can be planned without the host ever waiting for the GPU
        (``solver.WindowPipeline``).  Only valid when every source coordinate is an integer -- raw sensor columns are --
        because the compact plan is then built unconditionally; ``n`` stays an upper bound (out-of-image events are in
        no tile range and are never read) and ``counts()`` reports the numbers later."""
        lib = _hip.require_gpu()
        H, W = self.image_size
        th, tw = int(tile[0]), int(tile[1])
        tiles_y, tiles_x = (H + th - 1) // th, (W + tw - 1) // tw
        n_keys = tiles_y * tiles_x * th * tw
        dev = self.device
        n = self.n
        n_pad = (n + 3) // 4 * 4 + 4  # the tile-private kernels read 4 events (16 B) per lane
        xs, ys, dts, ps = (torch.zeros(n_pad, dtype=torch.float32, device=dev) for _ in range(4))
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        key_offsets = torch.empty(n_keys + 1, dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)  # [out-of-image sources, fractional sources]
        nbytes = int(lib.ebos_bin_scratch_bytes_events(n, H, W, th, tw))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _hip.on_device(dev):
            check(lib.ebos_bin_events_f32(ptr(self.x), ptr(self.y), ptr(self.dt), ptr(self.p), n, H, W, th, tw,
                                          ptr(xs), ptr(ys), ptr(dts), ptr(ps), ptr(perm), ptr(key_offsets), ptr(counts),
                                          counts.data_ptr() + 4, ptr(scratch), nbytes, stream_ptr()),
                  "ebos_bin_events")
        # (the work items depend on key_offsets only: enqueued in front of the read-back, which then carries their count as well)
        part_table = torch.empty(5 * tiles_y * tiles_x + 1, dtype=torch.int32, device=dev)
        with _hip.on_device(dev):
            check(lib.ebos_plan_parts(ptr(key_offsets), H, W, th, tw, _n_cu(dev), part_fixed_events(n, tiles_y * tiles_x, _n_cu(dev)),
                                      ptr(part_table), stream_ptr()), "ebos_plan_parts")
        used = fullest = None
        if deferred:
            dropped, fractional = 0, 0
        else:  # the ONE host read-back of the build: (outside the image, fractional sources, work items in use, fullest tile)
            dropped, fractional, used, fullest = _plan_facts(lib, key_offsets, H, W, th, tw, counts, part_table)
        kept = n - dropped
        src_perm = perm[:kept] if self.perm is None else self.perm[perm[:kept].long()]
        grp_offsets = cpix = cdt = None
        if fractional == 0 and th <= 256 and tw <= 256:
            # integer source coordinates (camera events): also build the compact 6 B/event plan
            n_tiles = tiles_y * tiles_x
            cap = kept + 3 * n_tiles + 8
            grp_offsets = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
            cpix = torch.zeros(cap, dtype=torch.int16, device=dev)
            cdt = torch.full((cap,), float("nan"), dtype=torch.float32, device=dev)
            with _hip.on_device(dev):
                check(lib.ebos_plan_compact_f32(ptr(xs), ptr(ys), ptr(dts), ptr(key_offsets), kept, H, W, th, tw,
                                                ptr(grp_offsets), ptr(cpix), ptr(cdt), cap, stream_ptr()), "ebos_plan_compact")
        # fractional source coordinates (undistorted events): the compact layout WITH the fractions per slot is built on the first
        # ``frac_compact`` access (the resident loops and the grid-sampling launches ask; API-parity operators and bench --fractional
        # never do and no longer pay the rank loop, the hot-pixel pass and 14 B/event: ADVICE r05)
        frac_pending = bool(fractional > 0 and th <= 256 and tw <= 256)
        out = EventPlan(xs[:kept], ys[:kept], dts[:kept], ps[:kept], self.image_size, kept, self.n_input,
                        (th, tw), key_offsets, src_perm, self.n_dropped + dropped, grp_offsets, cpix, cdt, part_table, self.dt_bound,
                        ref_fraction=self.ref_fraction, normalized_t=self.normalized_t)
        if self.bins is not None:
            if deferred:
                raise NotImplementedError('a time-aware plan (time_bin) needs the host read-back of the build: deferred=False, emit="full"')
            bins = torch.zeros(n_pad, dtype=torch.uint8, device=dev)  # permuted and padded like the other SoA arrays
            bins[:kept] = self.bins[perm[:kept].long()]
            out.bins, out.time_bin = bins[:kept], self.time_bin
        out.__dict__["_frac"] = None          # (grp_offsets, cpix, cdt, cfx, cfy) once built
        out.__dict__["_frac_pending"] = frac_pending
        out.__dict__["_counts"], out.__dict__["_deferred"] = counts, bool(deferred)
        out.__dict__["_parts_used"], out.__dict__["_fullest_tile"] = used, fullest
        return out

    def counts(self) -> Tuple[int, int]:
        """(events outside the image, events with fractional source coordinates) seen by ``bin`` -- a host read-back;
        a ``deferred`` plan with fractional sources is invalid and raises here."""
        c = self.__dict__.get("_counts")
        if c is None:
            return self.n_dropped, 0
        dropped, fractional = (int(v) for v in c.tolist())
        if fractional and self.__dict__.get("_deferred"):
            raise ValueError(f"{fractional} events have fractional source coordinates: a deferred plan needs integer ones")
        return dropped, fractional

    # ------------------------------------------------------------------------------------------
    def pixel_event_counts(self) -> torch.Tensor:
        """Events per source pixel [H, W] int64 (device), read off the plan's counting sort: the histogram of
        ``(trunc(x), trunc(y))`` that ``crop_event`` with integer bounds counts in.  No kernel of its own, no host read."""
        if not self.binned:
            raise ValueError("pixel_event_counts needs a binned plan (EventPlan.build(..., tile=...))")
        H, W = self.image_size
        th, tw = self.tile
        ty, tx = -(-H // th), -(-W // tw)
        per_key = (self.key_offsets[1:] - self.key_offsets[:-1]).to(torch.int64)       # keys are tile-major
        return per_key.reshape(ty, tx, th, tw).permute(0, 2, 1, 3).reshape(ty * th, tx * tw)[:H, :W]

    def patch_event_counts(self, patch_size: Tuple[int, int], sliding_window: Tuple[int, int]) -> torch.Tensor:
        """``len(crop_event(events, p.x_min, p.x_max, p.y_min, p.y_max))`` for every patch p of the grid at once:
        [gh, gw] int64 on the device.  Replaces the per-patch loop over the whole event array of the reference's
        patch solvers (src/solver/patch_eklt.py:118-126, src/solver/patch_eklt_pyramid2.py:215-228: O(n_patch * n))
        by box sums over the per-pixel histogram the plan already holds.  Exact for events inside the image, which is
        all a binned plan keeps (``n_dropped`` counts the others)."""
        import numpy as np

        from .types import patch_bounds

        H, W = self.image_size
        x0, x1, y0, y1 = (torch.from_numpy(np.clip(b, 0, lim)).to(self.device)
                          for b, lim in zip(patch_bounds((H, W), patch_size, sliding_window), (H, H, W, W)))
        x1, y1 = torch.maximum(x1, x0), torch.maximum(y1, y0)
        integral = torch.zeros((H + 1, W + 1), dtype=torch.int64, device=self.device)
        integral[1:, 1:] = self.pixel_event_counts().cumsum(0).cumsum(1)
        return (integral[x1[:, None], y1[None, :]] - integral[x0[:, None], y1[None, :]]
                - integral[x1[:, None], y0[None, :]] + integral[x0[:, None], y0[None, :]])

    # ------------------------------------------------------------------------------------------
    def iwe_dense(self, flow: torch.Tensor, pad: Tuple[int, int] = (0, 0), weight: Optional[torch.Tensor] = None,
                  halo: Optional[int] = DEFAULT_HALO, splits: Optional[int] = None) -> torch.Tensor:
        """Fused dense-flow warp + bilinear IWE: flow [2, H, W] -> iwe [H + 2 pad_h, W + 2 pad_w].
        ``halo=None`` (or an un-binned plan) selects the general global-atomic kernel; ``halo="auto"``: run-time windows per
        tile (``resolve_halo``)."""
        return _FusedIweDense.apply(flow, weight, self, (int(pad[0]), int(pad[1])), _norm_halo(self, halo), self.resolve_splits(splits))

    def iwe_2dof(self, thetas: torch.Tensor, pad: Tuple[int, int] = (0, 0), weight: Optional[torch.Tensor] = None,
                 halo: Optional[int] = DEFAULT_HALO, splits: Optional[int] = None) -> torch.Tensor:
        """Fused 2-DoF warp + bilinear IWE for K hypotheses: thetas [K, 2] -> iwes [K, h, w].
        Binned plans use the tile-private pipeline (|dt * theta| beyond ``halo`` spills, still correct)."""
        return _FusedIwe2Dof.apply(thetas, weight, self, (int(pad[0]), int(pad[1])), _norm_halo(self, halo), self.resolve_splits(splits))

    def variance_2dof(self, thetas: torch.Tensor, omit_boundary: bool = False, pad: Tuple[int, int] = (0, 0),
                      halo: int = DEFAULT_HALO, splits: Optional[int] = None, chunk: int = 16,
                      n_streams: int = 3) -> torch.Tensor:
        """Variance contrast of K translation hypotheses (the solver's outer sweep): [K, 2] -> [K].
        No gradient; images go into reused buffers.  The hypotheses are independent: they are dealt in chunks to ``n_streams``
        HIP streams -- the combine / finalize kernels of one chunk run in the wave slots that the one-workgroup-per-CU accumulate
        kernel of another leaves free -- and on a compact plan a chunk's accumulate pass is ONE persistent launch in which every
        workgroup keeps its tile and walks the chunk's hypotheses (``ebos_iwe_2dof_slab_batch_f32``: one LDS clear per launch, the
        next hypothesis' first events requested while the current image is stored).  ``halo="auto"``: run-time windows per tile."""
        lib = _hip.require_gpu()
        halo = _norm_halo(self, halo)
        if not _slab_ok(self, halo):
            return ops.image_variance(self.iwe_2dof(thetas, pad, None, None), omit_boundary)
        th = thetas.detach().to(device=self.device, dtype=torch.float32).contiguous()
        K = th.shape[0]
        H, W = self.image_size
        h, w = H + 2 * pad[0], W + 2 * pad[1]
        splits = self.resolve_splits(splits)
        out = torch.empty(K, dtype=torch.float32, device=self.device)
        n_streams = max(1, int(n_streams))
        chunk = max(1, min(int(chunk), (K + n_streams - 1) // n_streams))  # (a short sweep does not allocate 16 workspaces per lane)
        n_streams = max(1, min(n_streams, (K + chunk - 1) // chunk))
        persistent = self.compact and w % 4 == 0 and pad[1] % 4 == 0  # (what the batched pass asks of its images; else one launch per hypothesis)
        key = ("sweep", int(halo), int(splits), int(pad[0]), int(pad[1]), h, w, chunk, persistent)
        lanes = self.__dict__.setdefault("_sweep_lanes", {}).get(key)
        # (the size is asked of the library: _workspace() would allocate and cache a zero-filled workspace just to be measured)
        nws = int(lib.ebos_iwe_slab_workspace_bytes(H, W, self.tile[0], self.tile[1], int(halo), int(splits), pad[0], pad[1]))
        nws_al = (nws + 255) // 256 * 256
        with _hip.on_device(self.device):
            if lanes is None or len(lanes) < n_streams:  # streams, workspaces and image buffers live with the plan
                # one workspace per hypothesis of a chunk (36 MB each at 1280x720, tile 45x80, halo 32: 1.7 GB for 3 lanes of 16);
                # EventPlan.clear_cache() frees them
                lanes = [(torch.cuda.Stream(device=self.device),
                          torch.zeros((chunk if persistent else 1) * nws_al, dtype=torch.uint8, device=self.device),
                          torch.empty((chunk, h, w), dtype=torch.float32, device=self.device)) for _ in range(n_streams)]
                self.__dict__["_sweep_lanes"][key] = lanes
            cur = torch.cuda.current_stream(self.device)
            for st, _, _ in lanes[:n_streams]:
                st.wait_stream(cur)  # thetas / the plan were produced on the caller's stream
            for j, k0 in enumerate(range(0, K, chunk)):
                kc = min(chunk, K - k0)
                st, ws, buf = lanes[j % n_streams]
                if persistent:
                    check(lib.ebos_iwe_2dof_slab_batch_f32(*self._compact_ptrs(), ptr(self.key_offsets), self.n, th.data_ptr() + 8 * k0, kc,
                                                           H, W, self.tile[0], self.tile[1], int(halo), int(splits), pad[0], pad[1],
                                                           ptr(ws), nws_al, ptr(buf), 1, int(omit_boundary), out.data_ptr() + 4 * k0,
                                                           None, ptr(self.part_table), st.cuda_stream, None), "ebos_iwe_2dof_slab_batch")
                else:
                    check(lib.ebos_iwe_2dof_slab_f32(ptr(self.x), ptr(self.y), ptr(self.dt), None, *self._compact_ptrs(),
                                                     ptr(self.key_offsets), self.n, th.data_ptr() + 8 * k0, kc, H, W,
                                                     self.tile[0], self.tile[1], int(halo), int(splits), pad[0], pad[1],
                                                     ptr(ws), ws.numel(), ptr(buf), 1, int(omit_boundary),
                                                     out.data_ptr() + 4 * k0, None, ptr(self.part_table), st.cuda_stream),
                          "ebos_iwe_2dof_slab")
            for st, _, _ in lanes[:n_streams]:
                cur.wait_stream(st)
            th.record_stream(cur)
        return out

    def variance_and_grad_dense(self, flow: torch.Tensor, omit_boundary: bool = False, pad: Tuple[int, int] = (0, 0),
                                halo: int = DEFAULT_HALO, splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(variance [1], d variance / d flow [2, H, W]) in two launches' worth of Python, without building an autograd
        graph -- for callers that drive their own optimiser (the autograd engine alone costs more per backward() than
        both event kernels take).  Same kernels and results as ``contrast_dense(flow).backward()``."""
        flow32 = _check_flow(self, flow.detach())
        splits = self.resolve_splits(splits)
        pad = (int(pad[0]), int(pad[1]))
        halo = _norm_halo(self, halo)
        if not _slab_ok(self, halo):
            f = flow32.clone().requires_grad_(True)
            v = self.contrast_dense(f, "image_variance", omit_boundary, pad, halo)
            v.backward()
            return v.detach().reshape(1), f.grad
        out, d_flow = _run_dense_job(_dense_job(self, pad, halo, splits, omit_boundary), flow32, True)
        return out[:1], d_flow

    def variance_dense_many(self, flows: torch.Tensor, omit_boundary: bool = False, pad: Tuple[int, int] = (0, 0),
                            halo: int = DEFAULT_HALO, splits: Optional[int] = None, n_streams: int = 3) -> torch.Tensor:
        """Variance contrast of K independent dense-flow hypotheses (the trial loop of a sampler-driven search,
        src/solver/generative_max_likelihood.py:229-236): flows [K, 2, H, W] -> [K].  No gradient.  The evaluations are
        dealt to ``n_streams`` HIP streams with a workspace and an image buffer each, like ``variance_2dof``."""
        lib = _hip.require_gpu()
        if flows.dim() != 4 or tuple(flows.shape[1:]) != (2,) + tuple(self.image_size):
            raise ValueError(f"flows must be [K, 2, {self.image_size[0]}, {self.image_size[1]}], got {tuple(flows.shape)}")
        halo = _norm_halo(self, halo)
        if not _slab_ok(self, halo):
            return torch.stack([self.contrast_dense(f, "image_variance", omit_boundary, pad, halo).detach() for f in flows])
        fl = flows.detach().to(device=self.device, dtype=torch.float32).contiguous()
        K = fl.shape[0]
        H, W = self.image_size
        h, w = H + 2 * pad[0], W + 2 * pad[1]
        splits = self.resolve_splits(splits)
        out = torch.empty(K, dtype=torch.float32, device=self.device)
        n_streams = max(1, min(int(n_streams), K))
        key = ("dense_many", int(halo), int(splits), int(pad[0]), int(pad[1]), h, w)
        lanes = self.__dict__.setdefault("_sweep_lanes", {}).get(key)
        with _hip.on_device(self.device):
            if lanes is None or len(lanes) < n_streams:
                lanes = [(torch.cuda.Stream(device=self.device),
                          torch.zeros(_workspace(self, pad, halo, splits).numel(), dtype=torch.uint8, device=self.device),
                          torch.empty((h, w), dtype=torch.float32, device=self.device)) for _ in range(n_streams)]
                self.__dict__["_sweep_lanes"][key] = lanes
            cur = torch.cuda.current_stream(self.device)
            for st, _, _ in lanes[:n_streams]:
                st.wait_stream(cur)
            for k in range(K):
                st, ws, buf = lanes[k % n_streams]
                check(lib.ebos_iwe_dense_slab_f32(ptr(self.x), ptr(self.y), ptr(self.dt), None, *self._compact_ptrs(),
                                                  ptr(self.key_offsets), self.n, fl.data_ptr() + 8 * H * W * k, H, W, self.tile[0],
                                                  self.tile[1], int(halo), int(splits), pad[0], pad[1], ptr(ws), ws.numel(),
                                                  ptr(buf), 1, int(omit_boundary), out.data_ptr() + 4 * k, None,
                                                  ptr(self.part_table), st.cuda_stream), "ebos_iwe_dense_slab")
            for st, _, _ in lanes[:n_streams]:
                cur.wait_stream(st)
            fl.record_stream(cur)
        return out

    def contrast_dense(self, flow: torch.Tensor, cost: str = "image_variance", omit_boundary: bool = False,
                       pad: Tuple[int, int] = (0, 0), halo: Optional[int] = DEFAULT_HALO,
                       splits: Optional[int] = None, sign: float = 1.0, _eager_checked: bool = False) -> torch.Tensor:
        """Contrast of the IWE under ``flow`` (0-d tensor, raw contrast: callers apply the sign -- or pass ``sign=-1.0``, the
        ``direction="minimize"`` of the cost plugins, and get ``sign * contrast`` with its gradient straight from the kernels).
        Same value and gradient as ``cost(iwe_dense(flow))``, but the variance gradient is folded
        into the backward event kernel (no d_iwe image).

        One stream at a time per plan: the evaluation runs on a job cached on the plan (image, moments and workspace are shared
        between calls), so calls on the same plan from two streams must be ordered by the caller -- independent evaluations
        go through ``variance_dense_many`` / ``variance_2dof``, which give every stream its own buffers.  First order only:
        the gradient is produced with the value, ``backward`` is once-differentiable (``create_graph=True`` raises)."""
        halo = _norm_halo(self, halo)
        if cost not in ("image_variance", "gradient_magnitude"):
            raise KeyError(f"unknown contrast cost {cost!r}")
        if cost == "image_variance" or _slab_ok(self, halo):
            pad2, splits = (int(pad[0]), int(pad[1])), self.resolve_splits(splits)
            if _eager_checked or _eager_ok(self, flow, halo):
                # value and gradient by the one native call, handed back as a tensor whose ``.backward()`` -- when it is called on
                # the result itself, the objective idiom -- stores the gradient without entering the autograd engine (the engine's
                # thread hand-off around a Python backward costs more than both event kernels); any other use of the result
                # attaches the ordinary autograd node first (_EagerLoss)
                # A RAW contrast (sign = 1) is about to be negated by its caller -- contrast is maximised by minimising its negative:
                # the kernels produce -d contrast / d flow, and ``(-loss).backward()`` finds its factor already applied; negating the
                # 7.4 MB gradient afterwards is a launch of its own (55 -> 50 us per forward + backward at 10 M events).  A caller
                # that does differentiate the raw contrast pays that launch instead (_EagerLoss applies what is left to apply).
                sign = float(sign)
                spec = -1.0 if sign == 1.0 else sign
                out, d_flow = _run_dense_job(_dense_job(self, pad2, halo, splits, bool(omit_boundary)), flow, True, cost, spec)
                return _EagerLoss.wrap(out[1] if sign != 1.0 else out[0], flow, d_flow, sign, applied=spec)
            v = _FusedVarianceDense.apply(flow, self, pad2, bool(omit_boundary), halo, splits, cost)
            return v if sign == 1.0 else v * sign
        v = ops.gradient_magnitude(self.iwe_dense(flow, pad=pad, halo=halo, splits=splits), omit_boundary)
        return v if sign == 1.0 else v * sign

    # ------------------------------------------------------------------------------------------ second order
    def iwe_dense_jvp(self, flow: torch.Tensor, v: torch.Tensor, pad: Tuple[int, int] = (0, 0), halo="auto",
                      splits: Optional[int] = None, with_iwe: bool = True, weight: Optional[torch.Tensor] = None):
        """(iwe or None, tangent), float32 [H + 2 pad_h, W + 2 pad_w]: the IWE of ``flow`` [2, H, W] and its directional derivative
        u = d IWE(flow + e v) / de at e = 0 along ``v`` [2, H, W], from ONE pass over the events
        (``ebos_iwe_dense_tangent_tiled_f32``: a second LDS window per workgroup; ``with_iwe=False`` keeps the tangent's alone).  A
        plain function: no autograd graph.  ``halo``: a built halo of the plan's tile is used where its windows fit the LDS, else --
        and for ``"auto"`` -- the largest built halo of the tile whose windows fit as float64, failing that as float32
        (``ebos_iwe_multiref_fits`` with 2 windows, 1 without the IWE); displacements beyond it take the exact spill path.
        ``splits=None``: the slab route (``ebos_iwe_dense_tangent_slab_f32``) -- every tile stores its window(s) and a combine pass sums
        the windows that cover a cell in tile order, so the bits repeat from call to call, and with and without the IWE, wherever the
        windows are float64 and nothing spills.  Float32 windows -- two windows of (64, 64, 32), (32, 64, 32) and (32, 64, 48), the
        one window of (64, 64, 64) -- are summed by LDS float atomics in the order the hardware picks: the same images to rounding
        (1e-6 of the float64 image per cell, like float64 windows), but 0 of 10 repeated calls repeated the first call's bits on
        70 x 135 with 30 000 events (MI355X, tests/test_gpu_hvp_tiles.py, which runs every built triple).  ``splits=k``: k work
        items per tile on the atomic flush (``ebos_iwe_dense_tangent_tiled_f32``), whose sums over overlapping windows meet in
        float atomics: the same images to rounding.  NotImplementedError for an un-binned, lean or deferred plan, a tile without a fitting built halo and per-event
        weights; ValueError for a ``flow`` / ``v`` that is not the plan's."""
        flow32, v32 = _check_hvp_operands(self, flow, v, weight, "iwe_dense_jvp")
        halo = _hvp_halo(self, halo, 2 if with_iwe else 1, "iwe_dense_jvp")
        return _launch_tangent(self, flow32, v32, (int(pad[0]), int(pad[1])), halo, splits, bool(with_iwe))

    def contrast_dense_hvp(self, flow: torch.Tensor, v: torch.Tensor, cost="image_variance", omit_boundary: bool = False,
                           blur_sigma: float = 0.0, pad: Tuple[int, int] = (0, 0), halo="auto", state: Optional[dict] = None,
                           splits: Optional[int] = None, weight: Optional[torch.Tensor] = None):
        """(value, d_flow, hv, state) of the raw contrast C(flow) as ``contrast_dense`` signs it: its value (0-d), its gradient and
        its Hessian applied to ``v`` (both [2, H, W] float32).  A plain function: no autograd graph, no double backward.

        Both contrasts are quadratic in the image (blur, Sobel stencil, boundary crop and unbiased variance are linear or quadratic),
        so the cost's Hessian applied to the tangent image u = J v is the cost's gradient map evaluated at u: with G1 = grad cost(IWE)
        and G2 = grad cost(u), ``ebos_iwe_dense_hvp_owner_bwd_f32`` sums J^T G2 (the Gauss-Newton part), the curvature of the bilinear
        weights against G1, and the gradient J^T G1, in one walk of every source pixel's run (no atomics: the same bits on every call
        for the same G1, G2).  ``cost``: a name or ``{name: weight}`` -- both maps are linear in the weights, so several costs share
        the event passes.  ``blur_sigma > 0``: the contrast of the 3-tap blurred image, ``blur^T(grad cost(blur(.)))``.

        ``state`` (returned; pass it back for another ``v`` at the SAME flow and options) carries what depends on ``flow`` alone -- the
        IWE, G1 or its affine map, value and gradient: such a call makes the tangent window only, skips the first cost pass and
        returns the state's value and ``d_flow``.  The tangent image comes from the slab route of ``iwe_dense_jvp`` with the state's
        halo.  Where that halo keeps two windows of the plan's tile as float64 -- tiles (64, 64) (halo 16 with ``"auto"``), (32, 32)
        and (16, 64) (halo 32), ``hvp_float64_tiles()`` -- both calls run float64 windows and the product from a reused state is the
        product without one bit for bit, as are repeated products, value and ``d_flow`` (an event beyond the halo takes the spill
        path's float atomics, and then the last bits may differ).  On tile (32, 64), and with an explicit halo 32 on (64, 64), the
        two windows of the first call are float32 (LDS float atomics) and the state's single window float64: every figure meets the
        same bars, but ``d_flow`` repeated its bits in 0 of 10 calls and the tangent image with the IWE is not the tangent image
        without it bit for bit, so ``hv`` from a reused state need not be either (MI355X, tests/test_gpu_hvp_tiles.py); the solver's
        second-order methods refuse such a tile.  ``splits`` as in
        ``iwe_dense_jvp``.  Refusals: ``iwe_dense_jvp``'s, KeyError for an unknown cost."""
        flow32, v32 = _check_hvp_operands(self, flow, v, weight, "contrast_dense_hvp")
        costs = _hvp_costs(cost)
        pad = (int(pad[0]), int(pad[1]))
        key = (tuple(costs.items()), bool(omit_boundary), float(blur_sigma), pad)
        if state is not None:
            if state.get("key") != key:
                raise ValueError("contrast_dense_hvp: state was made with other options (cost, omit_boundary, blur_sigma, pad)")
            halo = _hvp_halo(self, state["halo"], 1, "contrast_dense_hvp")
            _, u = _launch_tangent(self, flow32, v32, pad, halo, splits, False)
        else:
            halo = _hvp_halo(self, halo, 2, "contrast_dense_hvp")
            iwe, u = _launch_tangent(self, flow32, v32, pad, halo, splits, True)
            state = _hvp_state(iwe, costs, bool(omit_boundary), float(blur_sigma), key, halo)
        g2, affine, g_lo = _hvp_upstreams(state, u, costs, bool(omit_boundary), float(blur_sigma))
        d_flow, hv = _launch_hvp_owner(self, flow32, v32, pad, state["g1"], g2, affine, g_lo, state.get("d_flow") is None)
        if d_flow is not None:
            state["d_flow"] = d_flow
        return state["value"], state["d_flow"], hv, state

    # ------------------------------------------------------------------------------------------ multi-reference contrast
    def iwe_dense_multi(self, flow: torch.Tensor, directions, pad: Tuple[int, int] = (0, 0), halo=DEFAULT_HALO,
                        splits: Optional[int] = None, fused: Optional[bool] = None) -> torch.Tensor:
        """The IWEs of ``flow`` [2, H, W] at several reference times: ``directions`` holds 1 to 4 entries of ``'first' | 'middle' |
        'last' | 'before' | 'after' | float`` (``parse_direction``) -> iwes [K, H + 2 pad_h, W + 2 pad_w], entry k what a plan built
        with direction k gives from ``iwe_dense``.  Differentiable with respect to ``flow`` for any upstream [K, h, w].

        The plan's dt was made with reference fraction f (``ref_fraction``) and normalised time, so reference k is the scalar shift
        f - r_k of every dt.  ``fused=True``: ONE pass over the events makes all K images (``ebos_iwe_dense_multiref_tiled_f32``: K
        LDS windows per tile) and the backward is the owner kernel (``ebos_iwe_dense_multiref_owner_bwd_f32``: no atomics, the same
        bits on every call); ``halo`` is used where K windows of it fit the LDS, else the largest built halo of the plan's tile that
        does (``ebos_iwe_multiref_fits``).  ``fused=False``: the loop route, K calls of ``ebos_iwe_dense_tiled_f32`` and of
        ``ebos_iwe_dense_bwd_f32`` on ``dt + shift_k``.  ``fused=None``: the loop route where nothing fits, else
        ``MULTIREF_DEFAULT_FUSED``.  ``fused="slab"``: the K-image form of the tile-private pipeline
        (``ebos_iwe_dense_slab_multiref_f32``: the reference is an outer grid dimension, one LDS window per workgroup, two launches)
        with the tile-private backward ``ebos_iwe_dense_tiled_multiref_bwd_f32`` (one launch, no atomics, the same bits on every
        call); ``halo`` must be a built halo of the plan's tile (``_hip.slab_multiref_configs()``).  ValueError for ``'random'``, an
        empty list, more than 4 directions, and a plan without normalised time or without a reference fraction; NotImplementedError
        for an un-binned, lean or deferred plan."""
        return _KImages.apply(flow, self, _multiref_job(self, directions, pad, halo, splits, fused, "iwe_dense_multi"))

    def contrast_dense_multi(self, flow: torch.Tensor, directions, cost: str = "image_variance", omit_boundary: bool = False,
                             pad: Tuple[int, int] = (0, 0), halo=DEFAULT_HALO, splits: Optional[int] = None,
                             fused: Optional[bool] = None) -> torch.Tensor:
        """The multi-reference focus objective: the MEAN over the references of the raw contrast of ``iwe_dense_multi`` (0-d tensor),
        differentiable with respect to ``flow``.  For ``image_variance`` the K variances come from one ``ebos_image_variance_f32`` call
        and their gradients are folded into the event backward as an affine map per reference (no d_iwe images)."""
        if cost not in ("image_variance", "gradient_magnitude"):
            raise KeyError(f"unknown contrast cost {cost!r}")
        job = _multiref_job(self, directions, pad, halo, splits, fused, "contrast_dense_multi")
        if cost != "image_variance":
            return ops.gradient_magnitude(_KImages.apply(flow, self, job), omit_boundary).mean()
        if job.route == "slab":   # the variances come out of the combine pass; their gradients are folded into the backward kernel
            return _MultiRefSlabVariance.apply(flow, self, job, bool(omit_boundary))
        return _KImagesVariance.apply(flow, self, job, bool(omit_boundary))

    def variance_multi_value_and_grad(self, flow: torch.Tensor, directions, omit_boundary: bool = False, pad: Tuple[int, int] = (0, 0),
                                      halo=DEFAULT_HALO, splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean_k var(IWE_k(flow)) [0-d], its gradient d_flow [2, H, W]) on the ``fused="slab"`` route, without autograd: three
        launches (accumulate, combine with the K variances, the K-reference backward with the variance gradients folded in)."""
        job = _multiref_job(self, directions, pad, halo, splits, "slab", "variance_multi_value_and_grad")
        flow32 = _check_flow(self, flow)
        K = len(job.shifts)
        iwes, variances, moments = _launch_multiref_slab_fwd(self, flow32, job, 1, bool(omit_boundary))
        upstream = torch.full((1,), 1.0 / K, dtype=torch.float32, device=self.device)
        d_flow = _launch_multiref_slab_bwd(self, flow32, job, iwes, None, int(bool(omit_boundary)), moments, upstream)
        return variances.mean(), d_flow

    # ------------------------------------------------------------------------------------------ time-aware warp
    def iwe_voxel(self, voxel: torch.Tensor, pad: Tuple[int, int] = (0, 0), weight: Optional[torch.Tensor] = None,
                  halo: Optional[int] = DEFAULT_HALO, splits: Optional[int] = None) -> torch.Tensor:
        """Fused time-aware warp + bilinear IWE on a plan built with ``time_bin=T``: voxel [T, 2, H, W] -> iwe
        [H + 2 pad_h, W + 2 pad_w]; every event is displaced by the flow of its own time bin (``plan.bins``).  Differentiable
        with respect to the voxel and the weights.  A binned plan whose (tile, halo) is a built ``ebos_tiled_config`` takes the
        tiled kernel (LDS tile + halo, spill path beyond it: exact for any displacement), anything else -- ``halo=None``, an
        un-binned plan -- the general global-atomic kernel.  ``halo="auto"`` means the default built halo here."""
        return _FusedIweVoxel.apply(voxel, weight, self, (int(pad[0]), int(pad[1])), _voxel_halo(self, halo), self.resolve_splits(splits))

    def contrast_voxel(self, voxel: torch.Tensor, cost: str = "image_variance", omit_boundary: bool = False,
                       pad: Tuple[int, int] = (0, 0), halo: Optional[int] = DEFAULT_HALO,
                       splits: Optional[int] = None) -> torch.Tensor:
        """Contrast of the time-aware IWE under ``voxel`` (0-d tensor, raw contrast), differentiable with respect to the voxel:
        the value and gradient of ``cost(iwe_voxel(voxel))`` through the existing cost kernels.  For ``image_variance`` the
        gradient 2 (IWE - mean) / (M - 1) is folded into the backward event kernel as an affine map of the IWE (no d_iwe image)."""
        if cost not in ("image_variance", "gradient_magnitude"):
            raise KeyError(f"unknown contrast cost {cost!r}")
        pad2, halo, splits = (int(pad[0]), int(pad[1])), _voxel_halo(self, halo), self.resolve_splits(splits)
        if cost == "image_variance":
            return _FusedVarianceVoxel.apply(voxel, self, pad2, bool(omit_boundary), halo, splits)
        return ops.gradient_magnitude(_FusedIweVoxel.apply(voxel, None, self, pad2, halo, splits), omit_boundary)

    def variance_voxel_value_and_grad(self, voxel: torch.Tensor, omit_boundary: bool = False, pad: Tuple[int, int] = (0, 0),
                                      halo="auto", upstream: float = 1.0,
                                      out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(var(IWE(voxel)) [1] f32, ``upstream`` * d var / d voxel [T, 2, H, W] f32) without an autograd node: the forward kernel of
        ``iwe_voxel``, the variance and its affine map, and the pixel-owner backward (``ebos_iwe_voxel_owner_bwd_f32``: no atomics,
        every cell written, the same bits on every call).  ``out``: a caller-owned contiguous float32 [T, 2, H, W] on the plan's
        device that is overwritten (it needs no clearing).  Needs a binned time-aware plan (``EventPlan.build(..,
        emit="full", time_bin=T, tile=..)``): the errors of ``contrast_voxel`` otherwise, ``NotImplementedError`` on an un-binned one."""
        lib = _hip.require_gpu()
        vox32 = _check_voxel(self, voxel)
        if not self.binned:
            raise NotImplementedError("variance_voxel_value_and_grad walks the runs of a binned plan: build it with a tile "
                                      "(contrast_voxel serves an un-binned one)")
        _refuse_deferred(self, "variance_voxel_value_and_grad")
        pad2 = (int(pad[0]), int(pad[1]))
        H, W = self.image_size
        T = int(vox32.shape[0])
        dev = self.device
        _check_out(out, (T, 2, H, W), dev)
        if out is None:
            out = torch.empty((T, 2, H, W), dtype=torch.float32, device=dev)
        iwe = _launch_iwe_voxel(self, vox32, None, pad2, _voxel_halo(self, halo), self.resolve_splits(None))
        value, moments = _image_variances(iwe[None], bool(omit_boundary))
        affine = _variance_affines(moments, torch.full((1,), float(upstream), dtype=torch.float32, device=dev))
        with _hip.on_device(dev):
            check(lib.ebos_iwe_voxel_owner_bwd_f32(ptr(self.x), ptr(self.y), ptr(self.dt), None, ptr(self.bins), ptr(self.key_offsets),
                                                   self.n, ptr(vox32), T, H, W, self.tile[0], self.tile[1], pad2[0], pad2[1], ptr(iwe),
                                                   ptr(affine), int(bool(omit_boundary)), ptr(out), stream_ptr()),
                  "ebos_iwe_voxel_owner_bwd")
        return value, out

    # ------------------------------------------------------------------------------------------ time-aware warp at K reference times
    def iwe_voxel_multi(self, voxel: torch.Tensor, directions, pad: Tuple[int, int] = (0, 0), halo: Optional[int] = DEFAULT_HALO,
                        splits: Optional[int] = None) -> torch.Tensor:
        """The time-aware IWEs of ``voxel`` [T, 2, H, W] at several reference times: ``directions`` holds 1 to 4 entries of ``'first' |
        'middle' | 'last' | 'before' | 'after' | float`` -> iwes [K, H + 2 pad_h, W + 2 pad_w], entry k what a plan built with
        direction k gives from ``iwe_voxel``.  Differentiable with respect to ``voxel`` for any upstream [K, h, w].

        Reference k is the scalar shift f - r_k of every dt (``multi_reference_shifts``); the bin of an event does not depend on it.
        One launch makes the K images (``ebos_iwe_voxel_multiref_tiled_f32``: the reference is an outer grid dimension of the tiled
        kernel of ``iwe_voxel``; where (tile, halo) is no built configuration, the general kernel reference by reference) and one
        launch the backward (``ebos_iwe_voxel_multiref_owner_bwd_f32``: an event is loaded and its flow gathered once for all
        references; no atomics, every cell of d_voxel written, the same bits on every call).  ValueError as ``multi_reference_shifts``
        and ``iwe_voxel``; NotImplementedError for an un-binned or deferred plan."""
        return _KImages.apply(voxel, self, _voxel_multi_job(self, directions, pad, halo, splits, "iwe_voxel_multi"))

    def contrast_voxel_multi(self, voxel: torch.Tensor, directions, cost: str = "image_variance", omit_boundary: bool = False,
                             pad: Tuple[int, int] = (0, 0), halo: Optional[int] = DEFAULT_HALO,
                             splits: Optional[int] = None) -> torch.Tensor:
        """The time-aware multi-reference focus objective: the MEAN over the references of the raw contrast of ``iwe_voxel_multi``
        (0-d tensor), differentiable with respect to ``voxel``.  For ``image_variance`` the K variances come from one
        ``ebos_image_variance_f32`` call and their gradients are folded into the event backward as an affine map per reference (no
        d_iwe images)."""
        if cost not in ("image_variance", "gradient_magnitude"):
            raise KeyError(f"unknown contrast cost {cost!r}")
        job = _voxel_multi_job(self, directions, pad, halo, splits, "contrast_voxel_multi")
        if cost == "image_variance":
            return _KImagesVariance.apply(voxel, self, job, bool(omit_boundary))
        return ops.gradient_magnitude(_KImages.apply(voxel, self, job), omit_boundary).mean()

    def variance_voxel_multi_value_and_grad(self, voxel: torch.Tensor, directions, omit_boundary: bool = False,
                                            pad: Tuple[int, int] = (0, 0), halo="auto", upstream: float = 1.0,
                                            out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean_k var(IWE_k(voxel)) [0-d] f32, ``upstream`` * its gradient d_voxel [T, 2, H, W] f32) without an autograd node: the
        K-image forward, one variance call, its K affine maps and the K-reference owner backward.  ``out``: a caller-owned contiguous
        float32 [T, 2, H, W] on the plan's device that is overwritten (it needs no clearing)."""
        job = _voxel_multi_job(self, directions, pad, halo, None, "variance_voxel_multi_value_and_grad")
        vox32 = _check_voxel(self, voxel)
        _hip.require_gpu()
        H, W = self.image_size
        T, K, dev = int(vox32.shape[0]), len(job.shifts), self.device
        _check_out(out, (T, 2, H, W), dev)
        iwes = job.forward(self, vox32)
        variances, moments = _image_variances(iwes, bool(omit_boundary))
        affine = _variance_affines(moments, torch.full((K,), float(upstream) / K, dtype=torch.float32, device=dev))
        d_voxel = job.backward(self, vox32, iwes, affine, int(bool(omit_boundary)), out=out)
        return variances.mean(), d_voxel


# ----------------------------------------------------------------------------------------------
INT32_MAX = 2 ** 31 - 1


class TimeAwarePlanStack(object):
    """B binned time-aware plans (``EventPlan.build(..., emit="full", time_bin=T, tile=...)``) of one geometry, stacked for the kernels
    that take the window from an outer grid dimension (``ebos_iwe_voxel_tiled_batch_f32``, ``ebos_iwe_voxel_owner_bwd_batch_f32``,
    ``ebos_cmax_voxel_solve_batch_f32``):

        x / y / dt / bins   the windows' SoA streams, in key order, one after the other
        key_offsets         int32 [B, n_keys + 1]: row b = window b's offsets + the window's base, so window b is the slice
                            key_offsets[b][0] .. key_offsets[b][n_keys] of the streams and a kernel needs no pointer table
        ns                  the windows' event counts (host)

    A stack of ONE plan copies nothing: its streams are views of the plan's and its offsets the plan's own, ``key_offsets[None]``.
    ValueError for a plan that is un-binned, deferred or without bins, for plans that differ in image size, tile, ``time_bin`` or
    warp direction (a plan keeps its direction as ``dt_bound``), and for more than INT32_MAX events in total.  An ``EventPlan`` holds no
    per-event weights (they are an argument of the operators), and the stacked kernels take none."""

    def __init__(self, plans: Sequence[EventPlan]):
        plans = list(plans)
        if not plans:
            raise ValueError("stack_time_aware: no plans")
        if len(plans) > _hip.CMAX_VOXEL_MAX_BATCH:
            raise ValueError(f"stack_time_aware: {len(plans)} plans, the batched kernels take at most {_hip.CMAX_VOXEL_MAX_BATCH}")
        first = plans[0]
        for b, plan in enumerate(plans):
            if not plan.binned or plan.x is None:
                raise ValueError(f"stack_time_aware: plan {b} is un-binned or lean; build it with emit='full', tile=..., time_bin=T")
            if plan.bins is None or plan.time_bin is None:
                raise ValueError(f"stack_time_aware: plan {b} holds no time bins (EventPlan.build(..., time_bin=T))")
            if plan.__dict__.get("_deferred"):
                raise ValueError(f"stack_time_aware: plan {b} is deferred (its build was not read back)")
            for what in ("image_size", "tile", "time_bin", "dt_bound"):
                a, v = getattr(first, what), getattr(plan, what)
                if (tuple(a) if isinstance(a, (tuple, list)) else a) != (tuple(v) if isinstance(v, (tuple, list)) else v):
                    name = "warp direction (dt_bound)" if what == "dt_bound" else what
                    raise ValueError(f"stack_time_aware: plan {b} differs from plan 0 in {name}: {v!r} against {a!r}")
            if plan.device != first.device:
                raise ValueError(f"stack_time_aware: plan {b} is on {plan.device}, plan 0 on {first.device}")
        self.ns = [int(p.n) for p in plans]
        if sum(self.ns) > INT32_MAX:
            raise ValueError(f"stack_time_aware: {sum(self.ns)} events in total are more than INT32_MAX")
        self.plans = plans
        self.image_size, self.tile, self.time_bin, self.dt_bound = first.image_size, tuple(first.tile), first.time_bin, first.dt_bound
        self.ref_fraction, self.normalized_t = first.ref_fraction, first.normalized_t
        self.n = sum(self.ns)
        if len(plans) == 1:   # the plan's own storage, no copies: the base is 0, so its offsets already index its streams
            self.x, self.y, self.dt, self.bins = (getattr(first, k)[:first.n] for k in ("x", "y", "dt", "bins"))
            self.key_offsets = first.key_offsets.to(torch.int32).contiguous()[None]
        else:
            self.x, self.y, self.dt = (torch.cat([getattr(p, k)[:p.n] for p in plans]).contiguous() for k in ("x", "y", "dt"))
            self.bins = torch.cat([p.bins[:p.n] for p in plans]).contiguous()
            bases = torch.tensor([sum(self.ns[:b]) for b in range(len(plans))], dtype=torch.int32, device=first.device)
            self.key_offsets = (torch.stack([p.key_offsets for p in plans]) + bases[:, None]).to(torch.int32).contiguous()

    @classmethod
    def from_raw(cls, cols: Sequence[torch.Tensor], ranges: Sequence[Tuple[int, int]], image_size: Tuple[int, int],
                 direction: Union[str, float], tile: Tuple[int, int], time_bin: int, roi=None, remove=None,
                 ticks_per_second: float = 1e6, normalize_t: bool = True) -> "TimeAwarePlanStack":
        """The stack of the windows ``ranges`` (half-open index ranges into the raw columns; they may overlap, come in any order and be
        empty) straight from the raw sensor columns ``cols`` = (col int16, row int16, t int32 | int64 ticks, pol) on the GPU, in one
        set of launches (``ebos_plan_time_aware_raw_batch``) and with ONE host read-back, the windows' event counts.  ``roi`` /
        ``remove``: the CROP and removal rectangles of ``evaluation.window_ingest_raw_batch`` (rows xmin, xmax, columns ymin, ymax).
        Window b holds what ``EventPlan.build(PreparedWindows.events(b), image_size, direction, normalize_t, tile=tile, emit="full",
        time_bin=time_bin)`` holds, up to the order of the events of one source pixel; ``plans[b]`` are views into the stack's
        buffers (their ``perm`` is the event's index inside its range, they carry no polarity stream, no compact layout and no work
        items).  Argument errors are raised before the GPU is asked for."""
        if isinstance(tile, str):
            if tile != "auto":
                raise ValueError("tile must be a (tile_h, tile_w) pair or 'auto'")
            tile = choose_tile(image_size)
        if tile is None:
            raise ValueError("TimeAwarePlanStack.from_raw builds binned plans: tile must be a (tile_h, tile_w) pair or 'auto'")
        time_bin = ops.check_time_bins(time_bin)
        cols = tuple(cols)
        if len(cols) not in (3, 4):
            raise ValueError("cols must be (col, row, t) or (col, row, t, pol)")
        col, row, t = cols[:3]
        for name, v, dts in (("col", col, (torch.int16,)), ("row", row, (torch.int16,)), ("t", t, (torch.int32, torch.int64))):
            if not isinstance(v, torch.Tensor) or v.dim() != 1 or v.dtype not in dts:
                raise ValueError(f"TimeAwarePlanStack.from_raw: {name} must be a 1-D tensor, dtype in {dts}; "
                                 f"got {tuple(getattr(v, 'shape', ()))} {getattr(v, 'dtype', type(v).__name__)}")
        n_total = int(t.shape[0])
        if int(col.shape[0]) != n_total or int(row.shape[0]) != n_total:
            raise ValueError("TimeAwarePlanStack.from_raw: the raw columns must be of equal length")
        ranges = [(int(b), int(e)) for b, e in ranges]
        if not ranges:
            raise ValueError("TimeAwarePlanStack.from_raw: no windows")
        if len(ranges) > _hip.CMAX_VOXEL_MAX_BATCH:
            raise ValueError(f"TimeAwarePlanStack.from_raw: {len(ranges)} windows, the batched kernels take at most {_hip.CMAX_VOXEL_MAX_BATCH}")
        for b, e in ranges:
            if not 0 <= b <= e <= n_total:
                raise IndexError(f"TimeAwarePlanStack.from_raw: range [{b}, {e}) outside the {n_total} events")
        total = sum(e - b for b, e in ranges)
        if total > INT32_MAX:
            raise ValueError(f"TimeAwarePlanStack.from_raw: {total} events in total are more than INT32_MAX")
        rects = []
        for name, r in (("roi", roi), ("remove", remove)):
            if r is not None:
                r = tuple(r[k] for k in ("xmin", "xmax", "ymin", "ymax")) if isinstance(r, dict) else tuple(r)
                if len(r) != 4 or any(int(v) != v for v in r):
                    raise ValueError(f"{name} must be four integers (xmin, xmax, ymin, ymax), got {r!r}")
                r = tuple(int(v) for v in r)
                if r[0] > r[1] or r[2] > r[3]:
                    raise ValueError(f"{name} must have xmin <= xmax and ymin <= ymax, got {r!r}")
            rects.append(r)
        roi, remove = rects
        H, W = int(image_size[0]), int(image_size[1])
        th, tw = int(tile[0]), int(tile[1])
        if not (0 < H <= 32767 and 0 < W <= 32767 and th > 0 and tw > 0):
            raise ValueError(f"TimeAwarePlanStack.from_raw: bad image size {H} x {W} or tile {th} x {tw}")
        ref_mode, frac = parse_direction(direction)
        lib = _hip.require_gpu()
        for name, v in (("col", col), ("row", row), ("t", t)):
            if not v.is_cuda:
                raise _hip.HipUnavailableError(f"TimeAwarePlanStack.from_raw: {name} must be on the GPU")
        col, row, t = col.contiguous(), row.contiguous(), t.contiguous()
        dev, B = t.device, len(ranges)
        n_keys = ((H + th - 1) // th) * ((W + tw - 1) // tw) * th * tw
        c_ranges = (C.c_int64 * (2 * B))(*[v for r in ranges for v in r])
        nbytes = int(lib.ebos_plan_time_aware_batch_scratch_bytes(c_ranges, B, H, W, th, tw))
        if nbytes == 0:
            raise ValueError(f"TimeAwarePlanStack.from_raw: bad geometry: {B} windows of {H} x {W}, tile {th} x {tw}")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # (zeroed: what lies behind the kept events, the eight spare elements of EventPlan.bin included, is read as padding)
        x, y, dt = (torch.zeros(total + 8, dtype=torch.float32, device=dev) for _ in range(3))
        bins = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
        perm = torch.zeros(total + 8, dtype=torch.int32, device=dev)
        key_local = torch.empty((B, n_keys + 1), dtype=torch.int32, device=dev)
        key_stacked = torch.empty((B, n_keys + 1), dtype=torch.int32, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
        tminmax = torch.empty((B, 2), dtype=torch.float64, device=dev)
        r4, m4 = roi or (0, 0, 0, 0), remove or (0, 0, 0, 0)
        with _hip.on_device(dev):
            check(lib.ebos_plan_time_aware_raw_batch(ptr(col), ptr(row), ptr(t), int(t.dtype == torch.int64), float(ticks_per_second),
                                                     n_total, c_ranges, B, int(roi is not None), *r4, int(remove is not None), *m4,
                                                     ref_mode, frac, int(bool(normalize_t)), time_bin, H, W, th, tw, ptr(x), ptr(y),
                                                     ptr(dt), ptr(bins), ptr(perm), total, ptr(key_local), ptr(key_stacked), n_keys + 1,
                                                     ptr(counts), ptr(tminmax), ptr(scratch), nbytes, stream_ptr()),
                  "ebos_plan_time_aware_raw_batch")
        host = counts.tolist()   # the ONE host read-back of the build: (kept, outside the image) x B
        self = object.__new__(cls)
        self.ns = [int(c[0]) for c in host]
        self.n = sum(self.ns)
        self.image_size, self.tile, self.time_bin = (H, W), (th, tw), time_bin
        self.dt_bound = dt_bound_for(direction, normalize_t)
        self.ref_fraction, self.normalized_t = ref_fraction_for(direction), bool(normalize_t)
        self.x, self.y, self.dt, self.bins, self.perm = x[:self.n], y[:self.n], dt[:self.n], bins[:self.n], perm[:self.n]
        self.key_offsets, self.tminmax = key_stacked, tminmax
        self.plans, base = [], 0
        for b, (n, dropped) in enumerate(host):
            plan = EventPlan(x[base:base + n], y[base:base + n], dt[base:base + n], None, (H, W), n, n + dropped, (th, tw), key_local[b],
                             perm[base:base + n], dropped, dt_bound=self.dt_bound, bins=bins[base:base + n], time_bin=time_bin,
                             ref_fraction=self.ref_fraction, normalized_t=self.normalized_t)
            plan.__dict__["_frac"], plan.__dict__["_frac_pending"] = None, False
            plan.__dict__["_counts"], plan.__dict__["_deferred"] = None, False
            plan.__dict__["_parts_used"], plan.__dict__["_fullest_tile"] = None, None
            self.plans.append(plan)
            base += n
        return self

    def __len__(self) -> int:
        return len(self.plans)

    @property
    def device(self) -> torch.device:
        return self.key_offsets.device

    def canonical(self) -> "TimeAwarePlanStack":
        """The same stack with the events of every source pixel's run in a canonical order: by (dt, x, y, bin).  A plan build leaves
        the order inside a run to its counting sort's atomic counter, and a kernel that adds in run order (the owner backwards)
        inherits it; on the canonical stack two builds of the same window give such a kernel the same bits.  Events that tie in all
        four are interchangeable.  The offsets are shared, the four streams are new tensors; ``perm`` is not carried.  Cached on the
        stack, and for a stack of one plan on that plan (a solver stacks the same plan again at every pyramid scale)."""
        cached = self.__dict__.get("_canonical")
        if cached is None and len(self.plans) == 1:
            cached = self.__dict__["_canonical"] = self.plans[0].__dict__.get("_canonical_stack")
        if cached is None:
            cached = self.__dict__["_canonical"] = object.__new__(type(self))
            cached.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("_canonical", "perm")})
            if self.n > 0:
                n = self.n
                x, y, dt, bins = self.x[:n], self.y[:n], self.dt[:n], self.bins[:n]
                # the run of an event: the stacked offsets are non-decreasing over (window, key)
                run = torch.searchsorted(self.key_offsets.reshape(-1).to(torch.int64), torch.arange(n, device=x.device), right=True)
                order = torch.arange(n, device=x.device)
                for key in (bins, y, x, dt, run):            # least significant first, each sort stable
                    order = order[torch.sort(key[order], stable=True)[1]]
                cached.x, cached.y, cached.dt, cached.bins = (v[order].contiguous() for v in (x, y, dt, bins))
            cached.__dict__["_canonical"] = cached
            if len(self.plans) == 1:
                self.plans[0].__dict__["_canonical_stack"] = cached
        return cached

    def ns_array(self):
        """The event counts as the ``int64_t`` host array of the C entry points."""
        return (C.c_int64 * len(self.ns))(*self.ns)


def _build_lean(source: int, events, raw, image_size, direction, normalize_t, tile, ticks_per_second, deferred):
    """``ebos_plan_lean``: compact plan straight from the window.  Returns None when the window cannot take it (fractional
    source coordinates, a geometry outside the LDS sort) -- the caller then runs the full build."""
    lib = _hip.require_gpu()
    H, W = int(image_size[0]), int(image_size[1])
    th, tw = int(tile[0]), int(tile[1])
    if th > 256 or tw > 256:
        return None
    ref_mode, frac = parse_direction(direction)
    if raw is None:
        dev, n = events.device, int(events.shape[0])
        col = row = t = None
    else:
        col, row, t = raw
        dev, n = t.device, int(t.shape[0])
    tiles_y, tiles_x = (H + th - 1) // th, (W + tw - 1) // tw
    n_tiles, n_keys = tiles_y * tiles_x, tiles_y * tiles_x * th * tw
    nbytes = int(lib.ebos_plan_lean_scratch_bytes(n, H, W, th, tw))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cap = n + 3 * n_tiles + 8
    key_offsets = torch.empty(n_keys + 1, dtype=torch.int32, device=dev)
    grp_offsets = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
    cpix = torch.empty(cap, dtype=torch.int16, device=dev)
    cdt = torch.empty(cap, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    part_table = torch.empty(5 * n_tiles + 1, dtype=torch.int32, device=dev)
    with _hip.on_device(dev):
        rc = lib.ebos_plan_lean(source, ptr(events), ptr(col), ptr(row), ptr(t), float(ticks_per_second), n, ref_mode, frac,
                                int(normalize_t), H, W, th, tw, ptr(key_offsets), ptr(grp_offsets), ptr(cpix), ptr(cdt), cap,
                                ptr(counts), None, ptr(scratch), nbytes, stream_ptr())
        if rc == -3:  # EBOS_ERR_UNSUPPORTED: geometry outside the LDS sort
            return None
        check(rc, "ebos_plan_lean")
        check(lib.ebos_plan_parts(ptr(key_offsets), H, W, th, tw, _n_cu(dev), part_fixed_events(n, n_tiles, _n_cu(dev)), ptr(part_table),
                                  stream_ptr()), "ebos_plan_parts")
    dropped, used, fullest = 0, None, None
    if not deferred:  # the one host read-back of the build: (outside the image, fractional sources, work items in use, fullest tile)
        dropped, fractional, used, fullest = _plan_facts(lib, key_offsets, H, W, th, tw, counts, part_table)
        if fractional:
            return None  # fractional (undistorted) source coordinates: the (x, y, dt) format of the full build
    plan = EventPlan(None, None, None, None, (H, W), n - dropped, n, (th, tw), key_offsets, None, dropped, grp_offsets, cpix, cdt,
                     part_table, dt_bound_for(direction, normalize_t), ref_fraction=ref_fraction_for(direction),
                     normalized_t=bool(normalize_t))
    plan.__dict__["_counts"], plan.__dict__["_deferred"], plan.__dict__["_parts_used"] = counts, bool(deferred), used
    plan.__dict__["_fullest_tile"] = fullest
    return plan


def _plan_facts(lib, key_offsets: torch.Tensor, H: int, W: int, th: int, tw: int, counts: torch.Tensor, part_table: torch.Tensor):
    """(outside the image, fractional sources, work items in use, events of the fullest tile): ``ebos_plan_facts`` + one 16-byte copy."""
    facts = torch.empty(4, dtype=torch.int32, device=key_offsets.device)
    with _hip.on_device(key_offsets.device):
        check(lib.ebos_plan_facts(ptr(key_offsets), H, W, th, tw, ptr(counts), ptr(part_table), ptr(facts), stream_ptr()), "ebos_plan_facts")
    return tuple(int(v) for v in facts.tolist())


def _check_flow(plan: EventPlan, flow: torch.Tensor) -> torch.Tensor:
    H, W = plan.image_size
    if tuple(flow.shape) != (2, H, W):
        raise ValueError(f"flow must be [2, {H}, {W}], got {tuple(flow.shape)}")
    if flow.device != plan.device:
        raise _hip.HipUnavailableError(f"flow is on {flow.device}, the event plan on {plan.device}")
    return flow.to(torch.float32).contiguous()


def _image_variances(images: torch.Tensor, omit: bool):
    """(variances [K] f32, moments [K, 2] f64) of images [K, h, w] by one cost-kernel call."""
    lib = _hip.require_gpu()
    K, h, w = images.shape
    out = torch.empty(K, dtype=torch.float32, device=images.device)
    moments = torch.empty((K, 2), dtype=torch.float64, device=images.device)
    nbytes = int(lib.ebos_cost_scratch_bytes(K))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=images.device)
    with _hip.on_device(images.device):
        check(lib.ebos_image_variance_f32(ptr(images), K, h, w, int(omit), ptr(out), ptr(moments), ptr(scratch), nbytes, stream_ptr()),
              "ebos_image_variance")
    return out, moments


def _variance_affines(moments: torch.Tensor, upstream: torch.Tensor) -> torch.Tensor:
    """affine [K, 2] f32: the gradient of variance k times upstream[k] as the map a_k IWE_k + c_k of its image, from moments [K, 2]."""
    lib = _hip.require_gpu()
    K = moments.shape[0]
    affine = torch.empty((K, 2), dtype=torch.float32, device=moments.device)
    with _hip.on_device(moments.device):
        check(lib.ebos_image_variance_affine_f32(ptr(moments), ptr(upstream), K, ptr(affine), stream_ptr()), "ebos_image_variance_affine")
    return affine


def _check_out(out: Optional[torch.Tensor], shape, device: torch.device) -> None:
    """A caller-owned gradient buffer of a ``..._value_and_grad`` method, where given."""
    if out is not None and (tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != device
                            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(shape)} on {device}")


def _slab_ok(plan: EventPlan, halo) -> bool:
    if not plan.binned or halo is None:
        return False
    built = _hip.slab_configs()
    if halo == "auto":
        return any((th, tw) == tuple(plan.tile) for th, tw, _ in built)
    return (plan.tile[0], plan.tile[1], _max_halo(int(halo))) in built


def _refuse_deferred(plan: EventPlan, what: str) -> None:
    """A deferred plan keeps ``n`` as an upper bound and zero-fills the tail of its SoA arrays: only the tile-range
    (slab / tiled) kernels skip that tail, the general kernels would read it as events at (0, 0)."""
    if plan.__dict__.get("_deferred"):
        raise NotImplementedError(f"{what}: a plan built with deferred=True only runs on the tile-private kernels "
                                  "(a built tile / halo configuration); rebuild it with deferred=False for the general path")
    if plan.lean:
        raise NotImplementedError(f"{what}: a lean plan (emit='compact') holds no SoA events: it only runs on the tile-private "
                                  "kernels (a built tile / halo configuration) with unit weights; build it with emit='full'")


def _workspace(plan: EventPlan, pad, halo, splits) -> torch.Tensor:
    """Zero-filled once; the kernels keep the spill section zero between calls."""
    lib = _hip.require_gpu()
    key = (int(halo), int(splits), int(pad[0]), int(pad[1]))
    cache = plan.__dict__.setdefault("_workspaces", {})
    if key not in cache:
        H, W = plan.image_size
        nbytes = int(lib.ebos_iwe_slab_workspace_bytes(H, W, plan.tile[0], plan.tile[1], key[0], key[1], key[2], key[3]))
        cache[key] = torch.zeros(nbytes, dtype=torch.uint8, device=plan.device)
    return cache[key]


class SlabBatch(object):
    """Independent windows of one geometry evaluated by ``ebos_iwe_slab_batch_f32``: accumulate, combine and finalize each run as
    one launch over (work item, window), 16 windows at a time -- the time windows of bos_event.py:144-220 when they are thin
    (BASELINE configs[3]: 2 M events), where per-launch fixed work and the gaps between launches dominate.

        batch = SlabBatch(plans, flows, patch=((24, 32), (24, 32)))   # flows: patch grids [2, gh, gw]; patch=None: dense [2, H, W]
        batch.run()                      # -> variances [n] (device), batch.iwes [n, h, w]
    The array of window descriptors is filled once; ``run`` is ONE C call.  Results are bit-identical to per-window calls."""

    def __init__(self, plans, flows, patch=None, pad=(0, 0), halo: int = DEFAULT_HALO, splits: Optional[int] = None,
                 omit_boundary: bool = False):
        lib = _hip.require_gpu()
        if not plans:
            raise ValueError("SlabBatch: no windows")
        p0 = plans[0]
        H, W = p0.image_size
        self.plans, self.flows = list(plans), [f.contiguous().float() for f in flows]
        if halo == "auto":  # one |dt| bound for the whole batch: the largest of the plans' (a plan without one: the built halo)
            bounds = [pl.dt_bound for pl in plans]
            if any(b is None for b in bounds):
                halo = max(hl for th, tw, hl in _hip.slab_configs() if (th, tw) == tuple(p0.tile))
            else:
                halo = int(lib.ebos_halo_auto(max(hl for th, tw, hl in _hip.slab_configs() if (th, tw) == tuple(p0.tile)), float(max(bounds))))
        self.pad, self.halo, self.omit = (int(pad[0]), int(pad[1])), int(halo), bool(omit_boundary)
        self.splits = p0.resolve_splits(splits)
        for pl, fl in zip(self.plans, self.flows):
            if pl.image_size != p0.image_size or pl.tile != p0.tile or not pl.compact or pl.device != p0.device:
                raise ValueError("SlabBatch: windows must share image size, tile and device, and be compact (unit-weight) plans")
            if pl.resolve_splits(splits) != self.splits:
                raise ValueError("SlabBatch: windows must share the work-item mode (all adaptive or all with the same split count)")
        if patch is None:
            self.grid = (0, 0, 0, 0, 0, 0)
            want = (2, H, W)
        else:
            (ph, pw), (sh, sw) = patch
            gh, gw = self.flows[0].shape[-2:]
            self.grid = (int(gh), int(gw), int(ph), int(pw), int(sh), int(sw))
            want = (2, gh, gw)
        for fl in self.flows:
            if tuple(fl.shape) != want:
                raise ValueError(f"SlabBatch: flow of shape {tuple(fl.shape)}, expected {want}")
        n = len(self.plans)
        dev = p0.device
        self.nws = int(lib.ebos_iwe_slab_workspace_bytes(H, W, p0.tile[0], p0.tile[1], self.halo, self.splits, *self.pad))
        self.workspaces = torch.zeros((n, (self.nws + 255) // 256 * 256), dtype=torch.uint8, device=dev)
        self.iwes = torch.empty((n, H + 2 * self.pad[0], W + 2 * self.pad[1]), dtype=torch.float32, device=dev)
        self.variances = torch.empty(n, dtype=torch.float32, device=dev)
        self.moments = torch.empty((n, 2), dtype=torch.float64, device=dev)
        self.windows = (_hip.SlabWindow * n)()
        P = lambda t: None if t is None else t.data_ptr()
        for k, (pl, fl) in enumerate(zip(self.plans, self.flows)):
            w = self.windows[k]
            cp = pl._compact_ptrs()
            w.grp_offsets, w.cpix, w.cdt = cp[0], cp[1], cp[2]
            w.key_offsets, w.part_table, w.flow = P(pl.key_offsets), P(pl.part_table) if self.splits == 0 else None, P(fl)
            w.workspace, w.iwe = self.workspaces[k].data_ptr(), self.iwes[k].data_ptr()
            w.out_variance, w.moments = self.variances.data_ptr() + 4 * k, self.moments[k].data_ptr()
        self._lib, self._tile, self._size = lib, p0.tile, (H, W)

    def run(self, want_variance: bool = True, stream: Optional[int] = None, tail_stream: Optional[int] = None) -> torch.Tensor:
        """``tail_stream`` (a raw HIP stream of the caller's): the combine / finalize passes of each 16 windows run there, beside
        the accumulate pass of the next 16; the results are ordered on ``stream`` when the call returns either way."""
        H, W = self._size
        _hip.check(self._lib.ebos_iwe_slab_batch_f32(self.windows, len(self.plans), *self.grid, H, W, self._tile[0], self._tile[1],
                                                     self.halo, self.splits, self.pad[0], self.pad[1], self.workspaces.shape[1],
                                                     1 if want_variance else 0, 1 if self.omit else 0,
                                                     _hip.stream_ptr() if stream is None else stream, tail_stream),
                   "ebos_iwe_slab_batch")
        return self.variances


class _DenseJob(object):
    """``ebos_dense_job`` of one (plan, padding, halo, splits, omit_boundary) with the buffers it points at: filled once,
    after which an objective (+ gradient) evaluation is ONE C call with six arguments (``ebos_variance_dense_job_f32``)."""

    def __init__(self, plan: EventPlan, pad, halo, splits, omit):
        import ctypes as C

        H, W = plan.image_size
        self.ws = _workspace(plan, pad, halo, splits)
        self.iwe = torch.empty((H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
        self.moments = torch.empty((1, 2), dtype=torch.float64, device=plan.device)
        g, c, d = plan._compact_ptrs()
        self.struct = _hip.DenseJob(ptr(plan.x), ptr(plan.y), ptr(plan.dt), g, c, d, ptr(plan.key_offsets), plan.n, H, W,
                                    plan.tile[0], plan.tile[1], int(halo), int(splits), pad[0], pad[1], int(omit), ptr(self.ws),
                                    self.ws.numel(), ptr(plan.part_table), ptr(self.iwe), ptr(self.moments))
        self.ref = C.addressof(self.struct)
        self.index = plan.device.index
        self._gm = None

    def gm_buffers(self):
        """Scratch of the gradient-magnitude job: the gradient image and the Sobel pass's value partials (allocated on first use)."""
        if self._gm is None:
            lib = _hip.require_gpu()
            h, w = self.iwe.shape
            n = int(lib.ebos_gradient_magnitude_fused_partials(h, w))
            self._gm = (torch.empty_like(self.iwe), torch.empty(n, dtype=torch.float64, device=self.iwe.device), n)
        return self._gm


def _dense_job(plan: EventPlan, pad, halo, splits, omit) -> _DenseJob:
    key = ("job", int(pad[0]), int(pad[1]), int(halo), int(splits), bool(omit))
    cache = plan.__dict__.setdefault("_jobs", {})
    job = cache.get(key)
    if job is None:
        job = cache[key] = _DenseJob(plan, pad, halo, splits, omit)
    return job


_SIGNS = {}


def _sign_constant(device: torch.device, sign: float) -> torch.Tensor:
    """Device-resident f32 [1] holding ``sign`` (the ``upstream`` of a signed job), made once per (device, value)."""
    key = (device, float(sign))
    t = _SIGNS.get(key)
    if t is None:
        t = _SIGNS[key] = torch.full((1,), float(sign), dtype=torch.float32, device=device)
    return t


def _run_dense_job(job: _DenseJob, flow32: torch.Tensor, want_grad: bool, cost: str = "image_variance", sign: float = 1.0):
    """(out [2] = (contrast, sign * contrast), sign * d contrast / d flow [2, H, W] | None) in one native call: the variance (three
    launches) or the gradient magnitude (four: one Sobel pass yields the value partials and the gradient image,
    ``ebos_gradient_magnitude_dense_job_f32``).  ``sign`` (the direction of a cost) is applied INSIDE the kernels: no launch negates
    a scalar or scales the gradient field afterwards; without a gradient only out[0] is written."""
    lib = _hip.require_gpu()
    out = torch.empty(2, dtype=torch.float32, device=flow32.device)
    d_flow = torch.empty_like(flow32) if want_grad else None
    up = None if sign == 1.0 else _sign_constant(flow32.device, sign).data_ptr()
    scaled = out.data_ptr() + 4 if want_grad else None

    def call():
        if cost == "image_variance":
            return lib.ebos_variance_dense_job_signed_f32(job.ref, flow32.data_ptr(), out.data_ptr(), scaled, up, ptr(d_flow), stream_ptr())
        d_iwe, partials, n = job.gm_buffers()
        return lib.ebos_gradient_magnitude_dense_job_f32(job.ref, flow32.data_ptr(), out.data_ptr(), scaled, up, ptr(d_flow),
                                                         d_iwe.data_ptr(), partials.data_ptr(), n, stream_ptr())

    if _hip.current_device_index() == job.index:
        rc = call()
    else:
        with _hip.on_device(flow32.device):
            rc = call()
    check(rc, "ebos_variance_dense_job" if cost == "image_variance" else "ebos_gradient_magnitude_dense_job")
    return out, d_flow


def _launch_iwe_dense_slab(plan: EventPlan, flow32, weight, pad, halo, splits, want_variance=False, omit=False):
    """Tile-private forward: returns (iwe, variance [1] | None, moments [1, 2] | None)."""
    lib = _hip.require_gpu()
    H, W = plan.image_size
    ws = _workspace(plan, pad, halo, splits)
    iwe = torch.empty((H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
    out = torch.empty(1, dtype=torch.float32, device=plan.device) if want_variance else None
    moments = torch.empty((1, 2), dtype=torch.float64, device=plan.device) if want_variance else None
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_dense_slab_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight), *plan._compact_ptrs(),
                                          ptr(plan.key_offsets), plan.n,
                                          ptr(flow32), H, W, plan.tile[0], plan.tile[1], int(halo), int(splits), pad[0],
                                          pad[1], ptr(ws), ws.numel(), ptr(iwe), int(want_variance), int(omit), ptr(out),
                                          ptr(moments), ptr(plan.part_table), stream_ptr()), "ebos_iwe_dense_slab")
    return iwe, out, moments


def _launch_iwe_dense(plan: EventPlan, flow32: torch.Tensor, weight, pad, halo, splits) -> torch.Tensor:
    lib = _hip.require_gpu()
    H, W = plan.image_size
    if _slab_ok(plan, halo):
        return _launch_iwe_dense_slab(plan, flow32, weight, pad, halo, splits)[0]
    _refuse_deferred(plan, "iwe_dense")
    iwe = torch.zeros((H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
    with _hip.on_device(plan.device):
        if plan.binned and halo is not None:
            check(lib.ebos_iwe_dense_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight), ptr(plan.key_offsets),
                                               plan.n, ptr(flow32), H, W, plan.tile[0], plan.tile[1], int(halo), max(1, splits),
                                               pad[0], pad[1], ptr(iwe), stream_ptr()), "ebos_iwe_dense_tiled")
        else:
            check(lib.ebos_iwe_dense_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight), plan.n, ptr(flow32), H, W,
                                         W, pad[0], pad[1], ptr(iwe), stream_ptr()), "ebos_iwe_dense")
    return iwe


def _plan_weight(plan: EventPlan, weight: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Per-event weights are given in INPUT order; reorder them like the events."""
    if weight is None:
        return None
    if plan.__dict__.get("_deferred"):
        # a deferred plan does not know how many events it kept: the tail of `perm` is not defined
        raise NotImplementedError("per-event weights need a plan built with the host read-back (deferred=False)")
    if plan.lean:
        raise NotImplementedError("per-event weights need the SoA events and the permutation: build the plan with emit='full'")
    w = weight.to(device=plan.device, dtype=torch.float32).reshape(-1)
    if w.numel() != plan.n_input:
        raise ValueError(f"weight must have one entry per input event ({plan.n_input}), got {w.numel()}")
    w = w if plan.perm is None else w[plan.perm.long()]
    out = torch.zeros((plan.n + 3) // 4 * 4 + 4, dtype=torch.float32, device=plan.device)  # 16-byte loads: padded
    out[:plan.n] = w
    return out[:plan.n]


def _launch_dense_bwd(plan, flow32, weight_p, pad, g_image, affine, g_lo, want_dweight, halo=DEFAULT_HALO,
                      var_moments=None, upstream=None, splits=1):
    lib = _hip.require_gpu()
    H, W = plan.image_size
    d_w = torch.empty(plan.n, dtype=torch.float32, device=plan.device) if want_dweight else None
    if _slab_ok(plan, halo):  # tile-private backward: d_flow written with plain stores, no zero-fill
        d_flow = torch.empty((2, H, W), dtype=torch.float32, device=plan.device)
        adaptive = splits == 0 and plan.part_table is not None
        ws = _workspace(plan, pad, halo, 0) if adaptive else None
        with _hip.on_device(plan.device):
            check(lib.ebos_iwe_dense_tiled_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight_p), *plan._compact_ptrs(),
                                                   ptr(plan.key_offsets), plan.n, ptr(flow32), H, W, plan.tile[0], plan.tile[1], int(halo), pad[0],
                                                   pad[1], ptr(g_image), ptr(affine), g_lo, ptr(d_flow), ptr(d_w),
                                                   ptr(var_moments), ptr(upstream), None, ptr(ws), ws.numel() if adaptive else 0,
                                                   ptr(plan.part_table) if adaptive else None, stream_ptr()),
                  "ebos_iwe_dense_tiled_bwd")
        return d_flow, d_w
    _refuse_deferred(plan, "iwe_dense backward")
    if var_moments is not None:  # general kernels take the affine form
        affine = _variance_affines(var_moments, upstream)
    d_flow = torch.zeros((2, H, W), dtype=torch.float32, device=plan.device)
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_dense_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight_p), plan.n, ptr(flow32), H, W,
                                         W, pad[0], pad[1], ptr(g_image), ptr(affine), g_lo, int(plan.binned),
                                         ptr(d_flow), ptr(d_w), stream_ptr()), "ebos_iwe_dense_bwd")
    return d_flow, d_w


def _unpermute(plan: EventPlan, d_w: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(plan.n_input, dtype=d_w.dtype, device=d_w.device)
    if plan.perm is None:
        out.copy_(d_w)
    else:
        out[plan.perm.long()] = d_w
    return out


class _FusedIweDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, weight, plan, pad, halo, splits):
        flow32 = _check_flow(plan, flow)
        wp = _plan_weight(plan, weight)
        iwe = _launch_iwe_dense(plan, flow32, wp, pad, halo, splits)
        ctx.save_for_backward(flow32, wp if wp is not None else torch.empty(0))
        ctx.meta = (plan, pad, flow.dtype, weight.dtype if weight is not None else None, halo, splits)
        return iwe if flow.dtype == torch.float32 else iwe.to(flow.dtype)

    @staticmethod
    def backward(ctx, g):
        flow32, wp = ctx.saved_tensors
        plan, pad, fdt, wdt, halo, splits = ctx.meta
        wp = wp if wdt is not None else None
        need_w = wdt is not None and ctx.needs_input_grad[1]
        d_flow, d_w = _launch_dense_bwd(plan, flow32, wp, pad, g.to(torch.float32).contiguous(), None, 0, need_w, halo,
                                        splits=splits)
        d_weight = _unpermute(plan, d_w).to(wdt) if need_w else None
        return (d_flow.to(fdt) if ctx.needs_input_grad[0] else None), d_weight, None, None, None, None


# ----------------------------------------------------------------------------------------------
# multi-reference contrast: the IWEs of one flow at several reference times
# ----------------------------------------------------------------------------------------------
MULTIREF_MAX = _hip.MULTIREF_MAX
# fused=None where K windows fit the LDS: what tools/bench_multiref.py measured
MULTIREF_DEFAULT_FUSED = False


def multi_reference_fractions(directions) -> List[float]:
    """``directions`` (1 to 4 of 'first' | 'middle' | 'last' | 'before' | 'after' | float) -> their fractions of the window."""
    if isinstance(directions, (str, float, int)) or directions is None:
        raise ValueError(f"directions must be a list of 1 to {MULTIREF_MAX} reference times, got {directions!r}")
    directions = list(directions)
    if not 1 <= len(directions) <= MULTIREF_MAX:
        raise ValueError(f"directions must hold 1 to {MULTIREF_MAX} reference times, got {len(directions)}")
    out = []
    for d in directions:
        if isinstance(d, str) and d == "random":
            raise ValueError("directions: 'random' is no reference time of a multi-reference objective (its draw differs per call)")
        if isinstance(d, (int, float)) and not isinstance(d, bool):
            d = float(d)
        frac = float(parse_direction(d)[1])
        if frac != frac or frac in (float("inf"), float("-inf")):
            raise ValueError(f"directions: {d!r} is not a finite fraction of the window")
        out.append(frac)
    return out


def multi_reference_shifts(plan: "EventPlan", directions) -> List[float]:
    """The float32 shifts f - r_k that turn the plan's dt (reference fraction f) into the dt of every direction."""
    import numpy as np

    fracs = multi_reference_fractions(directions)
    if not plan.normalized_t:
        raise ValueError("a multi-reference objective needs a plan built with normalised time (normalize_t=True): only then is another "
                         "reference time a shift of dt that the host knows")
    if plan.ref_fraction is None:
        raise ValueError("the plan does not know the reference fraction of its dt (a 'random' direction): build it with 'first', "
                         "'middle', 'last', 'before', 'after' or a float")
    return [float(np.float32(plan.ref_fraction - r)) for r in fracs]


class _KImagesJob(NamedTuple):
    """K images of a plan, one per reference time, and the route that makes them (``_ROUTES``: its operand check and its two
    launchers).  The operand x is the dense flow [2, H, W] on the dense routes and the flow voxel [T, 2, H, W] on "voxel"."""
    shifts: Tuple[float, ...]   # float32 values
    pad: Tuple[int, int]
    halo: Optional[int]         # the built halo of the route's forward kernel (None: the general kernel, reference by reference)
    splits: int
    route: str                  # "loop": K calls of the single kernels; "fused": K LDS windows per workgroup; "slab": the K-image
    #                             slab pipeline; "voxel": the time-aware kernels with the reference as an outer grid dimension

    @property
    def fused(self):
        """What ``fused=`` of ``iwe_dense_multi`` resolved to: False, True or "slab" (None on the voxel route, which has no such option)."""
        return {"loop": False, "fused": True, "slab": "slab"}.get(self.route)

    def check(self, plan: "EventPlan", x: torch.Tensor) -> torch.Tensor:
        """x as the contiguous float32 operand of the route, or the operand's refusal."""
        return _ROUTES[self.route][0](plan, x)

    def forward(self, plan: "EventPlan", x32: torch.Tensor) -> torch.Tensor:
        """-> images [K, h, w]."""
        return _ROUTES[self.route][1](plan, x32, self)

    def backward(self, plan: "EventPlan", x32: torch.Tensor, g_images: torch.Tensor, affine: Optional[torch.Tensor], g_lo: int,
                 **kw) -> torch.Tensor:
        """-> d_x = sum over the references of the event backward with upstream G_k = a_k g_images[k] + c_k."""
        return _ROUTES[self.route][2](plan, x32, self, g_images, affine, g_lo, **kw)


def _multiref_job(plan: "EventPlan", directions, pad, halo, splits, fused, what: str) -> _KImagesJob:
    shifts = tuple(multi_reference_shifts(plan, directions))
    if not plan.binned:
        raise NotImplementedError(f"{what} walks the runs of a binned plan: build it with a tile")
    _refuse_deferred(plan, what)
    if isinstance(fused, str) and fused == "slab":
        return _multiref_slab_job(plan, shifts, pad, halo, splits, what)
    if fused not in (None, True, False):
        raise ValueError(f"fused must be None, True, False or 'slab', got {fused!r}")
    lib = _hip.load_library()
    K = len(shifts)
    th, tw = int(plan.tile[0]), int(plan.tile[1])
    built = sorted(hl for a, b, hl in _hip.tiled_configs() if (a, b) == (th, tw))
    want = None if halo is None or halo == "auto" else _max_halo(int(halo))
    fit = [hl for hl in built if lib.ebos_iwe_multiref_fits(th, tw, hl, K) != 0]
    if want is not None and want in fit:
        fused_halo = want
    elif fit and (want is None or fused is True):
        fused_halo = max(fit)
    else:
        fused_halo = None
    if fused is True and fused_halo is None:
        raise NotImplementedError(f"{what}: no built halo of tile {(th, tw)} keeps {K} windows in the LDS (ebos_iwe_multiref_fits); "
                                  "fused=False runs the loop route")
    use_fused = fused_halo is not None and (MULTIREF_DEFAULT_FUSED if fused is None else fused)
    if use_fused:
        route_halo = fused_halo
    elif want is not None and want in built:
        route_halo = want
    elif built:
        route_halo = DEFAULT_HALO if DEFAULT_HALO in built and want is None else max(built)
    else:
        route_halo = None   # a tile without a tiled kernel: the general forward kernel, reference by reference
    return _KImagesJob(shifts, (int(pad[0]), int(pad[1])), route_halo, max(1, plan.resolve_splits(splits)), "fused" if use_fused else "loop")


def multiref_slab_halo(tile, halo) -> int:
    """The built halo the ``fused="slab"`` route runs ``tile`` with: ``halo`` itself where (tile, halo) is a built triple, the
    default (or else the largest) built halo of the tile for ``None`` / ``"auto"``; NotImplementedError names the built triples."""
    built_all = _hip.slab_multiref_configs()
    th, tw = int(tile[0]), int(tile[1])
    built = sorted(hl for a, b, hl in built_all if (a, b) == (th, tw))
    if halo is None or halo == "auto":
        if built:
            return DEFAULT_HALO if DEFAULT_HALO in built else max(built)
    elif _max_halo(int(halo)) in built:
        return _max_halo(int(halo))
    raise NotImplementedError(f"fused='slab': no multi-reference kernel is built for tile {(th, tw)} with halo {halo!r}; the built "
                              f"(tile_h, tile_w, halo) are {built_all}")


def _multiref_slab_job(plan: "EventPlan", shifts, pad, halo, splits, what: str) -> _KImagesJob:
    try:
        route_halo = multiref_slab_halo(plan.tile, halo)
    except NotImplementedError as e:
        raise NotImplementedError(f"{what}: {e}") from None
    return _KImagesJob(shifts, (int(pad[0]), int(pad[1])), route_halo, max(1, plan.resolve_splits(splits)), "slab")


def _multiref_workspace(plan: "EventPlan", K: int, pad, halo: int, splits: int) -> torch.Tensor:
    """K workspaces of the single form back to back, zero-filled once; the kernels keep the spill sections zero between calls."""
    lib = _hip.require_gpu()
    key = ("multiref", int(K), int(halo), int(splits), int(pad[0]), int(pad[1]))
    cache = plan.__dict__.setdefault("_workspaces", {})
    if key not in cache:
        H, W = plan.image_size
        nbytes = int(lib.ebos_iwe_slab_multiref_workspace_bytes(K, H, W, plan.tile[0], plan.tile[1], halo, splits, pad[0], pad[1]))
        if nbytes <= 0:
            raise RuntimeError(f"ebos_iwe_slab_multiref_workspace_bytes refused K={K} tile={plan.tile} halo={halo} splits={splits}")
        cache[key] = torch.zeros(nbytes, dtype=torch.uint8, device=plan.device)
    return cache[key]


def _launch_multiref_slab_fwd(plan: "EventPlan", flow32: torch.Tensor, job: _KImagesJob, want_variance: int, omit: bool):
    """-> (iwes [K, h, w], variances [K] | None, moments [K, 2] f64 | None); every output is overwritten by the kernels."""
    lib = _hip.require_gpu()
    H, W = plan.image_size
    K, pad = len(job.shifts), job.pad
    ws = _multiref_workspace(plan, K, pad, job.halo, job.splits)
    iwes = torch.empty((K, H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
    variances = torch.empty(K, dtype=torch.float32, device=plan.device) if want_variance else None
    moments = torch.empty((K, 2), dtype=torch.float64, device=plan.device) if want_variance else None
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_dense_slab_multiref_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32), H, W,
                                                   plan.tile[0], plan.tile[1], job.halo, job.splits, pad[0], pad[1], _c_shifts(job.shifts), K,
                                                   ptr(ws), ws.numel(), ptr(iwes), int(want_variance), int(omit), ptr(variances),
                                                   ptr(moments), stream_ptr()), "ebos_iwe_dense_slab_multiref")
    return iwes, variances, moments


def _launch_multiref_slab_bwd(plan: "EventPlan", flow32: torch.Tensor, job: _KImagesJob, g_images: torch.Tensor,
                              affine: Optional[torch.Tensor], g_lo: int, var_moments: Optional[torch.Tensor] = None,
                              upstream: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_flow [2, H, W] (every cell written) from a generic upstream (``g_images``, ``affine``) or the folded variance gradient
    (``g_images`` = the IWEs, ``var_moments`` [K, 2], ``upstream`` [1])."""
    lib = _hip.require_gpu()
    H, W = plan.image_size
    K, pad = len(job.shifts), job.pad
    d_flow = torch.empty((2, H, W), dtype=torch.float32, device=plan.device) if out is None else out
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_dense_tiled_multiref_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32),
                                                        H, W, plan.tile[0], plan.tile[1], job.halo, pad[0], pad[1], _c_shifts(job.shifts),
                                                        K, ptr(g_images), ptr(affine), int(g_lo), ptr(var_moments), ptr(upstream), None,
                                                        ptr(addend), ptr(d_flow), stream_ptr()), "ebos_iwe_dense_tiled_multiref_bwd")
    return d_flow


class _MultiRefSlabVariance(torch.autograd.Function):
    """mean_k var(IWE_k(flow)) on the slab route: the K variances and their moments come out of the combine pass, and the backward
    kernel folds 2 (IWE_k - mean_k) / (M - 1) in per reference -- no d_iwe images, no cost or affine launch."""

    @staticmethod
    def forward(ctx, flow, plan, job, omit):
        flow32 = _check_flow(plan, flow)
        iwes, variances, moments = _launch_multiref_slab_fwd(plan, flow32, job, 1, omit)
        ctx.save_for_backward(flow32, iwes, moments)
        ctx.meta = (plan, job, int(omit), flow.dtype)
        return variances.mean().to(flow.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        flow32, iwes, moments = ctx.saved_tensors
        plan, job, omit, fdt = ctx.meta
        upstream = (g.to(torch.float32).reshape(1) / iwes.shape[0]).contiguous()
        d_flow = _launch_multiref_slab_bwd(plan, flow32, job, iwes, None, omit, moments, upstream)
        return d_flow.to(fdt), None, None, None


def _multiref_dt(plan: "EventPlan", shift: float) -> torch.Tensor:
    """``plan.dt + shift`` in float32 (the loop route's event times of one reference), kept on the plan."""
    cache = plan.__dict__.setdefault("_multiref_dts", {})
    t = cache.get(shift)
    if t is None:
        t = cache[shift] = plan.dt if shift == 0.0 else (plan.dt + shift).contiguous()
    return t


def _c_shifts(shifts):
    return (C.c_float * len(shifts))(*shifts)


def _launch_multiref_fwd(plan: "EventPlan", flow32: torch.Tensor, job: _KImagesJob) -> torch.Tensor:
    lib = _hip.require_gpu()
    H, W = plan.image_size
    K, pad = len(job.shifts), job.pad
    iwes = torch.zeros((K, H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
    with _hip.on_device(plan.device):
        if job.route == "fused":
            check(lib.ebos_iwe_dense_multiref_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32),
                                                        H, W, plan.tile[0], plan.tile[1], job.halo, job.splits, pad[0], pad[1],
                                                        _c_shifts(job.shifts), K, ptr(iwes), stream_ptr()),
                  "ebos_iwe_dense_multiref_tiled")
            return iwes
        for k, shift in enumerate(job.shifts):
            dt_k = _multiref_dt(plan, shift)
            if job.halo is not None:
                check(lib.ebos_iwe_dense_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(dt_k), None, ptr(plan.key_offsets), plan.n, ptr(flow32),
                                                   H, W, plan.tile[0], plan.tile[1], job.halo, job.splits, pad[0], pad[1], ptr(iwes[k]),
                                                   stream_ptr()), "ebos_iwe_dense_tiled")
            else:
                check(lib.ebos_iwe_dense_f32(ptr(plan.x), ptr(plan.y), ptr(dt_k), None, plan.n, ptr(flow32), H, W, W, pad[0], pad[1],
                                             ptr(iwes[k]), stream_ptr()), "ebos_iwe_dense")
    return iwes


def _launch_multiref_bwd(plan: "EventPlan", flow32: torch.Tensor, job: _KImagesJob, g_images: torch.Tensor,
                         affine: Optional[torch.Tensor], g_lo: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_flow [2, H, W] = sum over the references of the event backward with upstream G_k = a_k g_images[k] + c_k."""
    lib = _hip.require_gpu()
    H, W = plan.image_size
    K, pad = len(job.shifts), job.pad
    with _hip.on_device(plan.device):
        if job.route == "fused":
            d_flow = torch.empty((2, H, W), dtype=torch.float32, device=plan.device) if out is None else out   # every cell is written
            check(lib.ebos_iwe_dense_multiref_owner_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n,
                                                            ptr(flow32), H, W, plan.tile[0], plan.tile[1], pad[0], pad[1],
                                                            _c_shifts(job.shifts), K, ptr(g_images), ptr(affine), int(g_lo), ptr(d_flow),
                                                            stream_ptr()), "ebos_iwe_dense_multiref_owner_bwd")
            return d_flow
        d_flow = torch.zeros((2, H, W), dtype=torch.float32, device=plan.device)
        for k, shift in enumerate(job.shifts):
            dt_k = _multiref_dt(plan, shift)
            check(lib.ebos_iwe_dense_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(dt_k), None, plan.n, ptr(flow32), H, W, W, pad[0], pad[1],
                                             ptr(g_images[k]), None if affine is None else ptr(affine[k]), int(g_lo), 1, ptr(d_flow),
                                             None, stream_ptr()), "ebos_iwe_dense_bwd")
    return d_flow


# ----------------------------------------------------------------------------------------------
# second order on the plain dense-flow warp: tangent image and Hessian-vector product
# ----------------------------------------------------------------------------------------------
def _check_hvp_operands(plan: EventPlan, flow: torch.Tensor, v: torch.Tensor, weight, what: str):
    """flow and v as the contiguous float32 operands of the second-order kernels, or the operator's refusal."""
    if not plan.binned:
        raise NotImplementedError(f"{what} walks the runs of a binned plan: build it with a tile")
    _refuse_deferred(plan, what)
    if weight is not None:
        raise NotImplementedError(f"{what}: per-event weights are not covered (the second-order kernels vote with unit weights)")
    H, W = plan.image_size
    for name, t in (("flow", flow), ("v", v)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (2, H, W):
            raise ValueError(f"{what}: {name} must be a tensor [2, {H}, {W}], got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        if not t.dtype.is_floating_point:
            raise ValueError(f"{what}: {name} must be a floating-point tensor, got {t.dtype}")
        if t.device != plan.device:
            raise _hip.HipUnavailableError(f"{name} is on {t.device}, the event plan on {plan.device}")
    return flow.detach().to(torch.float32).contiguous(), v.detach().to(torch.float32).contiguous()


def canonical_runs(plan: EventPlan) -> EventPlan:
    """The same binned full plan with the events of every source pixel's run in a canonical order: by (dt, x, y).  A plan build
    leaves the order inside a run to its counting sort's atomic counter, and a kernel that adds in run order (the owner kernels)
    inherits it; on the canonical plan two builds of the same window give such a kernel the same bits -- what a solver needs whose
    iterations amplify the last bit (``TimeAwarePlanStack.canonical`` does the same for a stack).  Events that tie in all three are
    interchangeable.  The offsets are shared, the event streams and the permutation are new tensors."""
    from dataclasses import replace

    if not plan.binned or plan.lean or plan.n == 0:
        return plan
    n = plan.n
    run = torch.searchsorted(plan.key_offsets.to(torch.int64), torch.arange(n, device=plan.device), right=True)
    order = torch.arange(n, device=plan.device)
    for key in (plan.y[:n], plan.x[:n], plan.dt[:n], run):   # least significant first, each sort stable
        order = order[torch.sort(key[order], stable=True)[1]]
    out = replace(plan, **{name: getattr(plan, name)[:n][order].contiguous() for name in ("x", "y", "dt", "p", "perm", "bins")
                           if getattr(plan, name) is not None})
    for k in ("_frac_pending", "_parts_used", "_fullest_tile"):   # what bin() learnt about the window; the caches stay behind
        if k in plan.__dict__:
            out.__dict__[k] = plan.__dict__[k]
    return out


def hvp_tile_halo(tile, halo, windows: int, what: str) -> Tuple[int, int]:
    """(halo, kind) of the tangent kernel on plans of ``tile`` for ``windows`` LDS windows (2 with the IWE, 1 without): the requested
    built halo if its windows fit, else a built halo of the tile that does (``_multiref_job``'s rule) -- the largest whose windows
    are float64 before the largest whose windows are float32: the tangent sums signed terms, and float32 windows are the slow ones
    (tile (64, 64), 2 M events: two float32 windows of halo 32 take 111 us, one float64 window 20) and the ones whose
    bits do not repeat.  ``kind``: ``ebos_iwe_multiref_fits`` of the choice, 2 = float64 windows, 1 = float32.  Needs the library,
    not a GPU."""
    lib = _hip.load_library()
    th, tw = int(tile[0]), int(tile[1])
    built_all = _hip.tiled_configs()
    kind = {hl: int(lib.ebos_iwe_multiref_fits(th, tw, hl, windows)) for a, b, hl in built_all if (a, b) == (th, tw)}
    fit = [hl for hl, k in kind.items() if k != 0]
    want = None if halo is None or halo == "auto" else _max_halo(int(halo))
    if want is not None and want in fit:
        return want, kind[want]
    if fit:
        best = max(fit, key=lambda hl: (kind[hl], hl))
        return best, kind[best]
    raise NotImplementedError(f"{what}: no built halo of tile {(th, tw)} keeps {windows} window(s) in the LDS (ebos_iwe_multiref_fits); "
                              f"the built (tile_h, tile_w, halo) are {built_all}")


def hvp_float64_tiles() -> list:
    """The built tiles on which ``contrast_dense_hvp`` keeps BOTH of its windows as float64 with some built halo -- where its value,
    gradient and product repeat their bits from call to call."""
    lib = _hip.load_library()
    return sorted({(th, tw) for th, tw, hl in _hip.tiled_configs() if lib.ebos_iwe_multiref_fits(th, tw, hl, 2) == 2})


def _hvp_halo(plan: EventPlan, halo, windows: int, what: str) -> int:
    """``hvp_tile_halo`` of the plan's tile: the built halo the tangent kernel runs with.  Displacements beyond it take the exact
    spill path."""
    return hvp_tile_halo(plan.tile, halo, windows, what)[0]


def _hvp_costs(cost) -> dict:
    costs = {cost: 1.0} if isinstance(cost, str) else {k: float(w) for k, w in dict(cost).items()}
    unknown = [k for k in costs if k not in ("image_variance", "gradient_magnitude")]
    if unknown or not costs:
        raise KeyError(f"unknown contrast cost {unknown[0] if unknown else cost!r}")
    return costs


def _launch_tangent(plan: EventPlan, flow32: torch.Tensor, v32: torch.Tensor, pad, halo: int, splits, with_iwe: bool):
    """``splits=None``: the slab route (``ebos_iwe_dense_tangent_slab_f32``: one work item per tile, the tiles' windows summed in a
    fixed order -- bits that repeat); an explicit ``splits >= 1``: the atomic flush (``ebos_iwe_dense_tangent_tiled_f32``) with that
    many work items per tile."""
    lib = _hip.require_gpu()
    H, W = plan.image_size
    th, tw = int(plan.tile[0]), int(plan.tile[1])
    windows = 2 if with_iwe else 1
    images = torch.zeros((windows, H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
    iwe = images[1] if with_iwe else None
    with _hip.on_device(plan.device):
        if splits is None:
            cache = plan.__dict__.setdefault("_workspaces", {})
            key = ("tangent", int(halo), windows)
            if key not in cache:   # (every slab that is read is written first: no zero-fill)
                cache[key] = torch.empty(int(lib.ebos_iwe_tangent_slab_workspace_bytes(H, W, th, tw, int(halo), windows)), dtype=torch.uint8,
                                         device=plan.device)
            ws = cache[key]
            check(lib.ebos_iwe_dense_tangent_slab_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32),
                                                      ptr(v32), H, W, th, tw, int(halo), pad[0], pad[1], ptr(ws), ws.numel(), ptr(iwe),
                                                      ptr(images[0]), stream_ptr()), "ebos_iwe_dense_tangent_slab")
        else:
            check(lib.ebos_iwe_dense_tangent_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32),
                                                       ptr(v32), H, W, th, tw, int(halo), max(1, plan.resolve_splits(splits)), pad[0],
                                                       pad[1], ptr(iwe), ptr(images[0]), stream_ptr()), "ebos_iwe_dense_tangent_tiled")
    return iwe, images[0]


def _launch_hvp_owner(plan: EventPlan, flow32, v32, pad, g1, g2, affine, g_lo: int, want_grad: bool):
    """-> (d_flow or None, hv), [2, H, W] each, every cell written."""
    lib = _hip.require_gpu()
    H, W = plan.image_size
    hv = torch.empty((2, H, W), dtype=torch.float32, device=plan.device)
    d_flow = torch.empty((2, H, W), dtype=torch.float32, device=plan.device) if want_grad else None
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_dense_hvp_owner_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32),
                                                   ptr(v32), H, W, plan.tile[0], plan.tile[1], pad[0], pad[1], ptr(g1), ptr(g2),
                                                   ptr(affine), int(g_lo), ptr(d_flow), ptr(hv), stream_ptr()),
              "ebos_iwe_dense_hvp_owner_bwd")
    return d_flow, hv


def _hvp_affine_route(costs: dict, blur_sigma: float) -> bool:
    """The variance contrast of the un-blurred image: its gradient map is an affine map of the image, folded into the owner kernel."""
    return set(costs) == {"image_variance"} and blur_sigma == 0.0


def _cost_value_and_grad_map(img: torch.Tensor, costs: dict, omit: bool, blur_sigma: float):
    """(sum_c w_c C_c(blur(img)) [0-d], its gradient map with respect to img [h, w]) through the cost kernels and their ``_grad``
    kernels, the blur pass and its backward.  The costs are quadratic in img, so the map is linear in it: evaluated at a tangent image
    it is the cost's Hessian applied to that image."""
    from .event_image_converter import EventImageConverter

    leaf = img.detach().requires_grad_(True)
    with torch.enable_grad():
        x = EventImageConverter._gaussian_blur3(leaf, blur_sigma) if blur_sigma > 0 else leaf
        value = None
        for name, wgt in costs.items():
            term = wgt * (ops.image_variance if name == "image_variance" else ops.gradient_magnitude)(x, omit)
            value = term if value is None else value + term
        (g,) = torch.autograd.grad(value, leaf)
    return value.detach(), g.contiguous()


def _hvp_state(iwe: torch.Tensor, costs: dict, omit: bool, blur_sigma: float, key, halo: int) -> dict:
    """What ``contrast_dense_hvp`` keeps of a flow: the IWE, the first upstream image (G1, or the image with its affine map), the value."""
    state = {"key": key, "halo": int(halo), "iwe": iwe, "d_flow": None}
    if _hvp_affine_route(costs, blur_sigma):
        wgt = costs["image_variance"]
        out, moments = _image_variances(iwe[None], omit)
        state["upstream"] = torch.full((1,), wgt, dtype=torch.float32, device=iwe.device)
        state["affine1"] = _variance_affines(moments, state["upstream"])
        state["g1"], state["value"] = iwe, wgt * out[0]
    else:
        state["value"], state["g1"] = _cost_value_and_grad_map(iwe, costs, omit, blur_sigma)
    return state


def _hvp_upstreams(state: dict, u: torch.Tensor, costs: dict, omit: bool, blur_sigma: float):
    """-> (g2, affine (a1, c1, a2, c2) or None, g_lo): the second upstream image, the cost's gradient map at the tangent image."""
    if _hvp_affine_route(costs, blur_sigma):
        _, moments = _image_variances(u[None], omit)
        affine = torch.cat([state["affine1"], _variance_affines(moments, state["upstream"])]).reshape(4).contiguous()
        return u, affine, int(omit)
    return _cost_value_and_grad_map(u, costs, omit, blur_sigma)[1], None, 0


# ----------------------------------------------------------------------------------------------
# time-aware warp on a plan: the flow of an event's own time bin
# ----------------------------------------------------------------------------------------------
def _voxel_halo(plan: EventPlan, halo) -> Optional[int]:
    """The built halo the tiled voxel kernel runs with, or None for the general kernel: ``"auto"`` is the default built halo."""
    if halo is None or not plan.binned:
        return None
    halo = DEFAULT_HALO if halo == "auto" else _max_halo(int(halo))
    return halo if (plan.tile[0], plan.tile[1], halo) in _hip.tiled_configs() else None


def _check_voxel(plan: EventPlan, voxel: torch.Tensor) -> torch.Tensor:
    H, W = plan.image_size
    if plan.bins is None:
        raise ValueError('the plan holds no time bins: build it with EventPlan.build(..., emit="full", time_bin=T)')
    if voxel.dim() != 4 or tuple(voxel.shape[1:]) != (2, H, W):
        raise ValueError(f"voxel must be [T, 2, {H}, {W}], got {tuple(voxel.shape)}")
    if voxel.shape[0] != plan.time_bin:
        raise ValueError(f"the plan's bins were made for time_bin={plan.time_bin}, the voxel has {voxel.shape[0]} bins")
    if voxel.device != plan.device:
        raise _hip.HipUnavailableError(f"voxel is on {voxel.device}, the event plan on {plan.device}")
    return voxel.to(torch.float32).contiguous()


def _launch_iwe_voxel(plan: EventPlan, vox32: torch.Tensor, weight, pad, halo, splits) -> torch.Tensor:
    lib = _hip.require_gpu()
    _refuse_deferred(plan, "iwe_voxel")
    H, W = plan.image_size
    T = int(vox32.shape[0])
    iwe = torch.zeros((H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
    with _hip.on_device(plan.device):
        if halo is not None:
            check(lib.ebos_iwe_voxel_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight), ptr(plan.bins), ptr(plan.key_offsets),
                                               plan.n, ptr(vox32), T, H, W, plan.tile[0], plan.tile[1], int(halo), max(1, splits),
                                               pad[0], pad[1], ptr(iwe), stream_ptr()), "ebos_iwe_voxel_tiled")
        else:
            check(lib.ebos_iwe_voxel_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight), ptr(plan.bins), plan.n, ptr(vox32), T,
                                         H, W, W, pad[0], pad[1], ptr(iwe), stream_ptr()), "ebos_iwe_voxel")
    return iwe


def _launch_voxel_bwd(plan: EventPlan, vox32, weight_p, pad, g_image, affine, g_lo, want_dweight, var_moments=None, upstream=None,
                      sorted_: Optional[bool] = None):
    """d_voxel [T, 2, H, W] (and d_weight in plan order).  ``var_moments`` / ``upstream``: the variance's gradient as the affine
    map of ``g_image`` = the IWE (``ebos_image_variance_affine_f32``).  ``sorted_``: None = what the plan is."""
    lib = _hip.require_gpu()
    _refuse_deferred(plan, "iwe_voxel backward")
    H, W = plan.image_size
    T = int(vox32.shape[0])
    d_w = torch.empty(plan.n, dtype=torch.float32, device=plan.device) if want_dweight else None
    if var_moments is not None:
        affine = _variance_affines(var_moments, upstream)
    d_voxel = torch.zeros((T, 2, H, W), dtype=torch.float32, device=plan.device)
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_voxel_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(weight_p), ptr(plan.bins), plan.n, ptr(vox32), T,
                                         H, W, W, pad[0], pad[1], ptr(g_image), ptr(affine), g_lo,
                                         int(plan.binned if sorted_ is None else sorted_), ptr(d_voxel), ptr(d_w), stream_ptr()),
              "ebos_iwe_voxel_bwd")
    return d_voxel, d_w


class _FusedIweVoxel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, voxel, weight, plan, pad, halo, splits):
        vox32 = _check_voxel(plan, voxel)
        wp = _plan_weight(plan, weight)
        iwe = _launch_iwe_voxel(plan, vox32, wp, pad, halo, splits)
        ctx.save_for_backward(vox32, wp if wp is not None else torch.empty(0))
        ctx.meta = (plan, pad, voxel.dtype, weight.dtype if weight is not None else None)
        return iwe if voxel.dtype == torch.float32 else iwe.to(voxel.dtype)

    @staticmethod
    def backward(ctx, g):
        vox32, wp = ctx.saved_tensors
        plan, pad, vdt, wdt = ctx.meta
        wp = wp if wdt is not None else None
        need_w = wdt is not None and ctx.needs_input_grad[1]
        d_voxel, d_w = _launch_voxel_bwd(plan, vox32, wp, pad, g.to(torch.float32).contiguous(), None, 0, need_w)
        d_weight = _unpermute(plan, d_w).to(wdt) if need_w else None
        return (d_voxel.to(vdt) if ctx.needs_input_grad[0] else None), d_weight, None, None, None, None


class _FusedVarianceVoxel(torch.autograd.Function):
    """var(IWE(voxel)): the IWE by the fused time-aware kernel, the variance and its moments by the cost kernel; the backward
    event kernel reads the IWE through the variance's affine map, so no d_iwe image is made."""

    @staticmethod
    def forward(ctx, voxel, plan, pad, omit, halo, splits):
        _hip.require_gpu()
        vox32 = _check_voxel(plan, voxel)
        iwe = _launch_iwe_voxel(plan, vox32, None, pad, halo, splits)
        out, moments = _image_variances(iwe[None], omit)
        ctx.save_for_backward(vox32, iwe, moments)
        ctx.meta = (plan, pad, int(omit), voxel.dtype)
        return out[0].to(voxel.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        vox32, iwe, moments = ctx.saved_tensors
        plan, pad, omit, vdt = ctx.meta
        up = g.to(torch.float32).reshape(1).contiguous()
        d_voxel, _ = _launch_voxel_bwd(plan, vox32, None, pad, iwe, None, omit, False, moments, up)
        return d_voxel.to(vdt), None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# time-aware warp at K reference times: the voxel kernels with the reference as one more dimension
# ----------------------------------------------------------------------------------------------
def _voxel_multi_job(plan: "EventPlan", directions, pad, halo, splits, what: str) -> _KImagesJob:
    shifts = tuple(multi_reference_shifts(plan, directions))
    if plan.bins is None:
        raise ValueError('the plan holds no time bins: build it with EventPlan.build(..., emit="full", time_bin=T)')
    if not plan.binned:
        raise NotImplementedError(f"{what} walks the runs of a binned plan: build it with a tile")
    _refuse_deferred(plan, what)
    return _KImagesJob(shifts, (int(pad[0]), int(pad[1])), _voxel_halo(plan, halo), max(1, plan.resolve_splits(splits)), "voxel")


def _launch_iwe_voxel_multi(plan: "EventPlan", vox32: torch.Tensor, job: _KImagesJob) -> torch.Tensor:
    lib = _hip.require_gpu()
    H, W = plan.image_size
    T, K, pad = int(vox32.shape[0]), len(job.shifts), job.pad
    iwes = torch.zeros((K, H + 2 * pad[0], W + 2 * pad[1]), dtype=torch.float32, device=plan.device)
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_voxel_multiref_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.bins), ptr(plan.key_offsets), plan.n,
                                                    ptr(vox32), T, H, W, plan.tile[0], plan.tile[1], 0 if job.halo is None else job.halo,
                                                    job.splits, pad[0], pad[1], _c_shifts(job.shifts), K, ptr(iwes), stream_ptr()),
              "ebos_iwe_voxel_multiref_tiled")
    return iwes


def _launch_voxel_multi_bwd(plan: "EventPlan", vox32: torch.Tensor, job: _KImagesJob, g_images: torch.Tensor,
                            affine: Optional[torch.Tensor], g_lo: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_voxel [T, 2, H, W] = sum over the references of the event backward with upstream G_k = a_k g_images[k] + c_k."""
    lib = _hip.require_gpu()
    H, W = plan.image_size
    T, K, pad = int(vox32.shape[0]), len(job.shifts), job.pad
    d_voxel = torch.empty((T, 2, H, W), dtype=torch.float32, device=plan.device) if out is None else out   # every cell is written
    with _hip.on_device(plan.device):
        check(lib.ebos_iwe_voxel_multiref_owner_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.bins), ptr(plan.key_offsets),
                                                        plan.n, ptr(vox32), T, H, W, plan.tile[0], plan.tile[1], pad[0], pad[1],
                                                        _c_shifts(job.shifts), K, ptr(g_images), ptr(affine), int(g_lo), ptr(d_voxel),
                                                        stream_ptr()), "ebos_iwe_voxel_multiref_owner_bwd")
    return d_voxel


_ROUTES = {   # route of a _KImagesJob -> (operand check, forward launcher, backward launcher)
    "loop": (_check_flow, _launch_multiref_fwd, _launch_multiref_bwd),
    "fused": (_check_flow, _launch_multiref_fwd, _launch_multiref_bwd),
    "slab": (_check_flow, lambda plan, flow32, job: _launch_multiref_slab_fwd(plan, flow32, job, 0, False)[0], _launch_multiref_slab_bwd),
    "voxel": (_check_voxel, _launch_iwe_voxel_multi, _launch_voxel_multi_bwd),
}


class _KImages(torch.autograd.Function):
    """The K images of a job, differentiable with respect to its operand for any upstream [K, h, w]."""

    @staticmethod
    def forward(ctx, x, plan, job):
        x32 = job.check(plan, x)
        images = job.forward(plan, x32)
        ctx.save_for_backward(x32)
        ctx.meta = (plan, job, x.dtype)
        return images if x.dtype == torch.float32 else images.to(x.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x32,) = ctx.saved_tensors
        plan, job, xdt = ctx.meta
        d_x = job.backward(plan, x32, g.to(torch.float32).contiguous(), None, 0)
        return d_x.to(xdt), None, None


class _KImagesVariance(torch.autograd.Function):
    """mean_k var(image_k) of a job: the K variances and their moments by one cost-kernel call; the event backward reads the images
    through the variances' affine maps, so no d_iwe image is made."""

    @staticmethod
    def forward(ctx, x, plan, job, omit):
        x32 = job.check(plan, x)
        images = job.forward(plan, x32)
        out, moments = _image_variances(images, omit)
        ctx.save_for_backward(x32, images, moments)
        ctx.meta = (plan, job, int(omit), x.dtype)
        return out.mean().to(x.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x32, images, moments = ctx.saved_tensors
        plan, job, omit, xdt = ctx.meta
        K = images.shape[0]
        affine = _variance_affines(moments, (g.to(torch.float32).reshape(1) / K).repeat(K).contiguous())
        d_x = job.backward(plan, x32, images, affine, omit)
        return d_x.to(xdt), None, None, None


def _eager_ok(plan: EventPlan, flow: torch.Tensor, halo) -> bool:
    """The objective idiom's short cut applies to a float32 leaf of the plan's own shape and device that wants its gradient, has no
    tensor hooks (they fire inside the engine), with grad mode on, on a tile-private configuration."""
    return (type(flow) is torch.Tensor or type(flow) is torch.nn.Parameter) and flow.requires_grad and flow.is_leaf and \
        torch.is_grad_enabled() and flow.dtype == torch.float32 and flow.is_contiguous() and flow.device == plan.device and \
        tuple(flow.shape) == (2,) + tuple(plan.image_size) and not flow._backward_hooks and \
        not getattr(flow, "_post_accumulate_grad_hooks", None) and _slab_ok(plan, halo)


class _AttachGrad(torch.autograd.Function):
    """The autograd node of an already computed (value, gradient) pair: what _EagerLoss turns into when it is used as anything
    but the direct target of ``backward()``.  ``scale``: the Python factor the value has been multiplied with since."""

    @staticmethod
    def forward(ctx, flow, value, d_flow, scale):
        ctx.save_for_backward(d_flow)
        ctx.scale = scale
        return value.detach()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (d_flow,) = ctx.saved_tensors
        return d_flow * (g.to(torch.float32) * ctx.scale), None, None, None


class _ConsumedGrad(torch.autograd.Function):
    """What an _EagerLoss turns into once ``backward()`` has handed its gradient over: an ordinary tensor that still prints,
    copies, compares and enters arithmetic like any result whose graph has been freed -- only a SECOND differentiation raises,
    with the engine's own wording."""

    @staticmethod
    def forward(ctx, flow, value):
        return value.detach()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("Trying to backward through the graph a second time: contrast_dense produced its gradient with the "
                           "value and backward() has already handed it to flow.grad. Evaluate the objective again (it is one "
                           "native call), or pass retain_graph=True to the first backward().")


class _EagerLoss(torch.Tensor):
    """0-d result of ``contrast_dense`` whose gradient w.r.t. the (leaf) flow exists already.

    ``loss.backward()`` on the object itself -- or on ``-loss`` / ``k * loss`` / ``loss / k`` with a Python number, the sign and
    weight a caller applies to a contrast -- accumulates that gradient into ``flow.grad`` exactly as the engine would (set when
    ``None``, added otherwise; scaled by ``gradient`` when one is given) without running the engine.  Every other use -- arithmetic
    with tensors, ``torch.*`` functions, ``grad_fn`` / ``requires_grad`` queries, ``backward`` with ``inputs`` / ``create_graph``
    -- first attaches the ordinary autograd node (_AttachGrad) and proceeds on that tensor, so results and graphs are those of
    ``_FusedVarianceDense``.  ``item()`` / ``detach()`` / ``float()`` / f-strings / ``print`` / comparisons read the value.
    ``torch.autograd.grad(loss, flow)`` dispatches the same way.  One entry point does not consult ``__torch_function__``: the
    FUNCTION ``torch.autograd.backward([loss])`` on the bare result raises ("does not require grad") instead of running -- use the
    method, or any expression of the result beyond a sign / Python weight (``loss + 0.0``).

    A result and its scaled descendants (``-loss``, ``k * loss``) share ONE gradient cell: the first ``backward()`` among them
    consumes it for all (as the engine frees the graph they would share), after which each of them is an ordinary tensor whose
    second differentiation raises (_ConsumedGrad) and whose every other use -- ``print``, ``cpu``, ``clone``, arithmetic for
    logging -- works."""

    _VALUE_ONLY = {"item", "detach", "__float__", "__format__", "tolist", "__bool__", "__int__", "dim", "size", "numel", "__len__",
                   "__repr__", "__str__", "__lt__", "__le__", "__gt__", "__ge__", "__eq__", "__ne__", "lt", "le", "gt", "ge", "eq",
                   "ne", "isnan", "isfinite", "isinf"}

    @staticmethod
    def wrap(value: torch.Tensor, flow: torch.Tensor, d_flow: torch.Tensor, scale: float = 1.0, cell=None,
             applied: float = 1.0) -> "_EagerLoss":
        """``value`` = scale x contrast; ``d_flow`` = applied x d contrast / d flow (the kernels apply a cost's sign themselves)."""
        t = torch.Tensor._make_subclass(_EagerLoss, value)
        # flow, shared cell [gradient (None once handed over), the factor it already carries], attached tensor, factor of this object
        t._ebos = [flow, cell if cell is not None else [d_flow, float(applied)], None, scale]
        return t

    def _plain(self) -> torch.Tensor:
        with torch._C.DisableTorchFunctionSubclass():
            return self.as_subclass(torch.Tensor)

    def _attached(self) -> torch.Tensor:
        st = self._ebos
        if st[2] is None:
            if st[1][0] is None:  # consumed (by this object or a scaled relative): an ordinary tensor with a freed graph
                st[2] = _ConsumedGrad.apply(st[0], self._plain())
            else:
                st[2] = _AttachGrad.apply(st[0], self._plain(), st[1][0], st[3] / st[1][1])
        return st[2]

    def _scaled(self, k) -> "_EagerLoss":
        st = self._ebos
        if st[2] is not None or st[1][0] is None:  # already a graph node (or consumed): the ordinary path
            return self._attached() * k
        return _EagerLoss.wrap(self._plain() * k, st[0], None, st[3] * float(k), cell=st[1])

    def __neg__(self):
        return self._scaled(-1.0)

    def __mul__(self, other):
        return self._scaled(other) if isinstance(other, (int, float)) and not isinstance(other, bool) else self._attached() * other

    __rmul__ = __mul__

    def __truediv__(self, other):
        return self._scaled(1.0 / other) if isinstance(other, (int, float)) and not isinstance(other, bool) and other != 0 \
            else self._attached() / other

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        st = self._ebos
        flow, cell = st[0], st[1]
        if st[2] is not None or create_graph or inputs is not None or cell[0] is None or flow._backward_hooks or \
                getattr(flow, "_post_accumulate_grad_hooks", None):
            return self._attached().backward(gradient, retain_graph, create_graph, inputs)
        g, k = cell[0], st[3] / cell[1]  # (what is left to apply: nothing when the kernels applied this object's factor)
        with torch.no_grad():
            if gradient is not None:
                f = gradient.to(device=g.device, dtype=torch.float32) * k
            else:
                f = None if k == 1.0 else k
            if retain_graph:
                g = g * f if f is not None else g.clone()  # the cell keeps the unscaled gradient for the next backward()
            else:
                cell[0] = None  # consumed for this object AND its scaled relatives; the buffer now belongs to flow.grad
                if f is not None:
                    g.mul_(f)
            if flow.grad is None:
                flow.grad = g
            else:
                flow.grad.add_(g)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        value_only = getattr(func, "__name__", "") in cls._VALUE_ONLY
        conv = (lambda a: a._plain()) if value_only else (lambda a: a._attached())
        args, kwargs = _pytree.tree_map_only(_EagerLoss, conv, (tuple(args), kwargs))  # (also inside lists: torch.stack([loss, ...]))
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


class _FusedVarianceDense(torch.autograd.Function):
    """var(IWE(flow)).  On the tile-private configurations the gradient is produced WITH the value (one native call:
    accumulate, combine, finalize, tile-private backward with unit upstream) whenever the flow requires grad, and
    ``backward`` only scales it -- the interpreter and the autograd engine, not the kernels, bound this path (272 us
    against 65 us of kernels per fwd + bwd at 10 M events before)."""

    @staticmethod
    def forward(ctx, flow, plan, pad, omit, halo, splits, cost="image_variance"):
        _hip.require_gpu()
        fast = flow.dtype == torch.float32 and flow.is_contiguous() and flow.device == plan.device and \
            tuple(flow.shape) == (2,) + tuple(plan.image_size)
        flow32 = flow if fast else _check_flow(plan, flow)
        ctx.fdt = flow.dtype
        if _slab_ok(plan, halo):  # IWE + contrast (+ gradient) in one tile-private pipeline
            job = _dense_job(plan, pad, halo, splits, omit)
            out, d_flow = _run_dense_job(job, flow32, ctx.needs_input_grad[0], cost)
            ctx.eager = True
            if d_flow is not None:
                ctx.save_for_backward(d_flow)
            return out[0] if flow.dtype == torch.float32 else out[0].to(flow.dtype)
        ctx.eager = False
        iwe = _launch_iwe_dense(plan, flow32, None, pad, halo, splits)
        out, moments = _image_variances(iwe[None], omit)
        ctx.save_for_backward(flow32, iwe, moments)
        ctx.meta = (plan, pad, int(omit), halo, splits)
        return out[0].to(flow.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable  # the saved gradient is a constant: create_graph must raise, not drop terms
    def backward(ctx, g):
        if ctx.eager:
            (d_flow,) = ctx.saved_tensors
            d = d_flow * g.to(torch.float32)
            return (d if ctx.fdt == torch.float32 else d.to(ctx.fdt)), None, None, None, None, None, None
        flow32, iwe, moments = ctx.saved_tensors
        plan, pad, omit, halo, splits = ctx.meta
        up = g.to(torch.float32).reshape(1).contiguous()
        d_flow, _ = _launch_dense_bwd(plan, flow32, None, pad, iwe, None, omit, False, halo, moments, up, splits=splits)
        return d_flow.to(ctx.fdt), None, None, None, None, None, None


class _FusedIwe2Dof(torch.autograd.Function):
    @staticmethod
    def forward(ctx, thetas, weight, plan, pad, halo, splits):
        lib = _hip.require_gpu()
        if thetas.dim() != 2 or thetas.shape[1] != 2:
            raise ValueError(f"thetas must be [K, 2], got {tuple(thetas.shape)}")
        th32 = thetas.to(device=plan.device, dtype=torch.float32).contiguous()
        wp = _plan_weight(plan, weight)
        K = th32.shape[0]
        H, W = plan.image_size
        h, w = H + 2 * pad[0], W + 2 * pad[1]
        with _hip.on_device(plan.device):
            if _slab_ok(plan, halo):
                ws = _workspace(plan, pad, halo, splits)
                iwes = torch.empty((K, h, w), dtype=torch.float32, device=plan.device)
                check(lib.ebos_iwe_2dof_slab_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(wp), *plan._compact_ptrs(),
                                                 ptr(plan.key_offsets), plan.n, ptr(th32), K, H, W, plan.tile[0],
                                                 plan.tile[1], int(halo), int(splits), pad[0], pad[1], ptr(ws), ws.numel(),
                                                 ptr(iwes), 0, 0, None, None, ptr(plan.part_table), stream_ptr()),
                      "ebos_iwe_2dof_slab")
            else:
                _refuse_deferred(plan, "iwe_2dof")
                iwes = torch.zeros((K, h, w), dtype=torch.float32, device=plan.device)
                check(lib.ebos_iwe_2dof_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(wp), plan.n, ptr(th32), K, h, w,
                                            pad[0], pad[1], ptr(iwes), stream_ptr()), "ebos_iwe_2dof")
        ctx.save_for_backward(th32, wp if wp is not None else torch.empty(0))
        ctx.meta = (plan, pad, thetas.dtype, thetas.device, weight is not None, halo, splits)
        return iwes if thetas.dtype == torch.float32 else iwes.to(thetas.dtype)

    @staticmethod
    def backward(ctx, g):
        lib = _hip.require_gpu()
        th32, wp = ctx.saved_tensors
        plan, pad, tdt, tdev, has_w, halo, splits = ctx.meta
        K = th32.shape[0]
        H, W = plan.image_size
        h, w = H + 2 * pad[0], W + 2 * pad[1]
        g32 = g.to(torch.float32).contiguous()
        d_th = torch.zeros((K, 2), dtype=torch.float32, device=plan.device)
        with _hip.on_device(plan.device):
            if _slab_ok(plan, halo):
                ws = _workspace(plan, pad, halo, splits)
                check(lib.ebos_iwe_2dof_tiled_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(wp) if has_w else None,
                                                      *plan._compact_ptrs(), ptr(plan.key_offsets), plan.n, ptr(th32), K, H, W,
                                                      plan.tile[0], plan.tile[1], int(halo), pad[0], pad[1], ptr(g32), None, 0,
                                                      ptr(d_th), ptr(ws), ws.numel(), stream_ptr()), "ebos_iwe_2dof_tiled_bwd")
                return d_th.to(device=tdev, dtype=tdt), None, None, None, None, None
            check(lib.ebos_iwe_2dof_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(wp) if has_w else None, plan.n,
                                            ptr(th32), K, h, w, pad[0], pad[1], ptr(g32), None, 0, ptr(d_th),
                                            stream_ptr()), "ebos_iwe_2dof_bwd")
        return d_th.to(device=tdev, dtype=tdt), None, None, None, None, None
