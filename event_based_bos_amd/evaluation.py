"""The reference driver's per-frame evaluation of a recording (bos_event.py:109-220, ``evaluate_per_frames``), with the windows
batched and everything between the frame load and the error dicts kept on the device.

    config = utils.propagate_config(yaml_dict)
    events = RawEventStore("recording.npz")
    frames = FrameStore("frames/", "trigger_events.txt", "homography.txt", (720, 1280))
    solv = solver.collections[config["solver"]["method"]]((720, 1280), (720, 640), None, config["solver"])
    result = RecordingEvaluator(config, events, frames, solv, save_dir="out").run(max_batch=8)

writes the reference's ``flow_error_per_frame_with_mask.txt``, ``flow_error_per_frame_without_mask.txt`` and
``timestamps_per_frame.txt`` and returns the per-step dicts and their statistics.

``plan_evaluation`` restates the driver's index arithmetic on the host (no GPU): which frame pairs are evaluated and which slices
of the event columns each pair reads.  ``window_ingest_raw_batch`` (csrc/window_ingest.hip) turns the estimation slices of a batch
of steps into the solver's polarity images, the event masks of the masked error and the windows' time periods in one launch,
straight from the raw sensor columns; the generative solvers and ``ContrastMaximization`` take them through
``estimate_batch_prepared``.  A ``time_aware: {native: true}`` contrast maximisation with Adam builds the stacked time-aware plan of
a batch from the same columns (``TimeAwarePlanStack.from_raw``) and solves the batch in one loop; its other configurations run
``estimate`` on the windows' device events one after the other.  Any other registered solver is driven window by window through
``preprocess`` + ``estimate``.

``run(photometric=True)`` also asks whether the flows explain the frames: per step the photometric score
(``photometric.photometric_error_batch``) of the scaled estimate and of the frame-based flow on the two un-cropped frames, counted
inside the ``common_params`` rectangle, into ``photometric_per_frame.txt`` and ``photometric_reference_per_frame.txt``.

``run(pictures=True)`` also draws the driver's ten pictures per step (bos_event.py:202-207) on the device, batched
(``visualizer.render_step_batch``), and writes them under ``save_dir`` in the driver's order and under its file names.

Out of scope: ``method: openpiv`` / ``estimation_method: openpiv``, the visualizer's videos.
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip, event_filters, flow_error, frame_flow, photometric
from ._hip import check, ptr, stream_ptr

logger = logging.getLogger(__name__)

NOSE_RECT = (0, 120, 990, 1050)   # rows [0, 120) x columns [990, 1050): the driver's ``remove_nose`` rectangle
SUPPORTED_METHODS = ("opencv_flow", "opencv_flow_two_steps")
TEXT_WITH_MASK = "flow_error_per_frame_with_mask.txt"
TEXT_WITHOUT_MASK = "flow_error_per_frame_without_mask.txt"
TEXT_TIMESTAMPS = "timestamps_per_frame.txt"
TEXT_PHOTOMETRIC = "photometric_per_frame.txt"
TEXT_PHOTOMETRIC_REFERENCE = "photometric_reference_per_frame.txt"


# ------------------------------------------------------------------------------------------------ the plan (host)
@dataclass(frozen=True)
class EvalStep(object):
    """One frame pair of the evaluation loop.  ``run`` is False for a pair the driver skips (wrong cropped shape); such a step
    does not advance ``i_frame``."""
    i_frame: int
    i1: int
    i2: int
    t1: float
    t2: float                      # (after the max_time_per_event_batch cut, as the driver's timestamps file records it)
    gt_range: Tuple[int, int]      # event indices [begin, end) between the two frames
    est_range: Tuple[int, int]     # event indices [begin, end) the solver gets
    gt_time_scale: float
    run: bool = True


def _cropped_shape(shape, common: dict) -> Tuple[int, int]:
    """Shape of ``image[..., xmin:xmax, ymin:ymax]`` for an image of ``shape`` (Python's slice rules)."""
    h = len(range(*slice(common["xmin"], common["xmax"]).indices(int(shape[-2]))))
    w = len(range(*slice(common["ymin"], common["ymax"]).indices(int(shape[-1]))))
    return h, w


def _frame_shape(frames, index: int) -> Tuple[int, int]:
    if hasattr(frames, "image_shape"):
        return tuple(frames.image_shape(index))
    return tuple(frames.load_image(index)[0].shape)


def plan_evaluation(config: dict, events, frames) -> List[EvalStep]:
    """The steps of ``evaluate_per_frames`` (bos_event.py:117-184) for ``config`` (propagated), in the driver's order."""
    eval_config, common, data = config["evaluation"], config["common_params"], config["data"]
    cropped = (data["crop_height"], data["crop_width"])
    dt = eval_config["dt"]
    n_events = data["n_events_per_batch"] if "n_events_per_batch" in data else None
    max_dt = data["max_time_per_event_batch"] if "max_time_per_event_batch" in data else None
    n_all = len(events)
    steps, i_frame = [], 0
    for start, end in eval_config["time_list"]:
        ind_start = frames.time_to_image_index(start) + 1
        ind_end = frames.time_to_image_index(end) - dt
        for i1 in range(ind_start, ind_end):
            i2 = i1 + dt
            t1, t2 = frames.image_index_to_time(i1), frames.image_index_to_time(i2)
            run = _cropped_shape(_frame_shape(frames, i1), common) == cropped and _cropped_shape(_frame_shape(frames, i2), common) == cropped
            ind1, ind2 = events.time_to_index(t1), events.time_to_index(t2)
            gt_range = (max(ind1, 0), min(ind2, n_all))
            if max_dt is not None and t2 - t1 > max_dt:
                t2 = t1 + max_dt
                ind1, ind2 = events.time_to_index(t1), events.time_to_index(t2)
            if n_events is not None:
                if ind2 - ind1 < n_events:
                    insufficient = n_events - (ind2 - ind1)
                    ind1 -= insufficient // 2
                    ind2 += insufficient // 2
                elif ind2 - ind1 > n_events:
                    ind1 = ind2 - n_events
            est_range = (max(ind1, 0), min(ind2, n_all))
            steps.append(EvalStep(i_frame, i1, i2, t1, t2, gt_range, est_range, t2 - t1, run))
            i_frame += int(run)
    return steps


# ------------------------------------------------------------------------------------------------ batched window ingest
class PreparedWindows(object):
    """The event side of B windows on the device, as ``window_ingest_raw_batch`` leaves it.

    pol [B, 2, H, W] float64 ... positive / negative event counts (the solver's polarity image of the cropped window)
    mask [B, H, W] uint8 ... pixels with an event (``create_eventmask``)
    count [B] int64, t_min / t_max [B] float64 ... kept events and their first / last time; ``period`` = t_max - t_min
    """

    def __init__(self, pol, mask, count, t_min, t_max, cols=None, ranges=None, roi=None, remove=None, ticks_per_second=1e6,
                 period=None):
        self.pol, self.mask, self.count, self.t_min, self.t_max = pol, mask, count, t_min, t_max
        self.cols, self.ranges, self.roi, self.remove, self.ticks_per_second = cols, ranges, roi, remove, ticks_per_second
        self.period = (t_max - t_min) if period is None else period

    def __len__(self) -> int:
        return int(self.pol.shape[0])

    def slice(self, lo: int, hi: int) -> "PreparedWindows":
        return PreparedWindows(self.pol[lo:hi], self.mask[lo:hi], self.count[lo:hi], self.t_min[lo:hi], self.t_max[lo:hi], self.cols,
                               None if self.ranges is None else self.ranges[lo:hi], self.roi, self.remove, self.ticks_per_second,
                               self.period[lo:hi])

    def events(self, i: int) -> torch.Tensor:
        """Window i's kept events as a device float64 [n, 4] array (row, col, t in seconds, p): what ``load_event`` ->
        ``remove_event`` -> CROP gives, built on the device from the raw columns."""
        if self.cols is None or self.ranges is None:
            raise ValueError("these windows do not carry their raw columns")
        lo, hi = self.ranges[i]
        col, row, t, p = (c[lo:hi] for c in self.cols)
        keep = _keep_mask(col, row, self.roi, self.remove)
        ev = torch.stack([row.double(), col.double(), _seconds(t, self.ticks_per_second), p.double()], dim=1)
        return ev if keep is None else ev[keep]


def _seconds(ticks: torch.Tensor, ticks_per_second: float) -> torch.Tensor:
    """ticks / ticks_per_second in float64 as numpy divides (a tensor divisor: torch turns the division of a device tensor by a
    Python number into a multiplication by its reciprocal, which rounds differently)."""
    t = ticks.double()
    return t / torch.full_like(t, float(ticks_per_second))


def _keep_mask(col, row, roi, remove) -> Optional[torch.Tensor]:
    keep = None
    if roi is not None:
        x0, x1, y0, y1 = roi
        keep = (row >= x0) & (row < x1) & (col >= y0) & (col < y1)
    if remove is not None:
        x0, x1, y0, y1 = remove
        out = ~((row >= x0) & (row < x1) & (col >= y0) & (col < y1))
        keep = out if keep is None else keep & out
    return keep


def _rect(r, name: str) -> Optional[Tuple[int, int, int, int]]:
    if r is None:
        return None
    r = tuple(r[k] for k in ("xmin", "xmax", "ymin", "ymax")) if isinstance(r, dict) else tuple(r)
    if len(r) != 4 or any(int(v) != v for v in r):
        raise ValueError(f"{name} must be four integers (xmin, xmax, ymin, ymax), got {r!r}")
    return tuple(int(v) for v in r)


def window_ingest_raw_batch(cols: Sequence[torch.Tensor], ranges, image_shape, roi=None, remove=None,
                            ticks_per_second: float = 1e6) -> PreparedWindows:
    """``ebos_window_ingest_raw_batch``: the polarity images, event masks, counts and time ranges of B windows in one launch.

    Args:
        cols ... (col int16, row int16, t int32 | int64, pol uint8 | bool) device columns, as ``RawEventStore.load_raw`` returns.
        ranges ... B pairs (begin, end) into the columns; they may overlap and may be empty.
        image_shape ... (H, W) of the sensor.
        roi ... the solver's CROP rectangle (xmin, xmax = rows, ymin, ymax = columns; tuple or dict) or None.
        remove ... an optional rectangle whose events are dropped (the driver's ``remove_nose``).
    Fractional coordinates are not handled here: columns that are not int16 raise ``ValueError`` (route such windows through
    ``estimate_batch``)."""
    col, row, t, pol = cols
    for name, c in (("col", col), ("row", row)):
        if not isinstance(c, torch.Tensor) or c.dtype != torch.int16:
            raise ValueError(f"{name} must be an int16 tensor of sensor pixels (fractional coordinates take the estimate_batch path), "
                             f"got {getattr(c, 'dtype', type(c).__name__)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"t must hold int32 or int64 ticks, got {t.dtype}")
    if pol.dtype == torch.bool:
        pol = pol.view(torch.uint8)
    if pol.dtype != torch.uint8:
        raise ValueError(f"pol must be uint8 or bool, got {pol.dtype}")
    n = int(t.shape[0])
    if any(c.dim() != 1 or int(c.shape[0]) != n for c in (col, row, t, pol)):
        raise ValueError("the raw columns must be 1-D and of equal length")
    pairs = [(int(a), int(b)) for a, b in ranges]
    if not pairs:
        raise ValueError("ranges holds no window")
    for a, b in pairs:
        if not 0 <= a <= n or not 0 <= b <= n:
            raise ValueError(f"range ({a}, {b}) leaves the {n} events of the columns")
    pairs = [(a, max(a, b)) for a, b in pairs]
    H, W = (int(v) for v in image_shape)
    roi, remove = _rect(roi, "roi"), _rect(remove, "remove")
    lib = _hip.require_gpu()
    dev = t.device
    if not t.is_cuda:
        raise ValueError("the raw columns must be on the GPU (RawEventStore.load_raw)")
    col, row, t, pol = (c.contiguous() for c in (col, row, t, pol))
    B = len(pairs)
    r4 = roi or (0, 0, 0, 0)
    m4 = remove or (0, 0, 0, 0)
    nbytes = int(lib.ebos_window_ingest_scratch_bytes(B, H, W, int(roi is not None), *r4))
    if nbytes == 0:
        raise ValueError(f"bad geometry: {B} windows of {H} x {W}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rng = torch.tensor(pairs, dtype=torch.int64).to(dev, non_blocking=True)
    out_pol = torch.empty((B, 2, H, W), dtype=torch.float64, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    count = torch.empty(B, dtype=torch.int64, device=dev)
    t_min, t_max = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
    with _hip.on_device(dev):
        check(lib.ebos_window_ingest_raw_batch(ptr(col), ptr(row), ptr(t), int(t.dtype == torch.int64), ptr(pol), n,
                                               float(ticks_per_second), ptr(rng), B, max(b - a for a, b in pairs), H, W,
                                               int(roi is not None), *r4, int(remove is not None), *m4, ptr(out_pol), ptr(mask),
                                               ptr(count), ptr(t_min), ptr(t_max), ptr(scratch), nbytes, stream_ptr(dev)),
              "ebos_window_ingest_raw_batch")
    return PreparedWindows(out_pol, mask, count, t_min, t_max, (col, row, t, pol), pairs, roi, remove, float(ticks_per_second))


# ------------------------------------------------------------------------------------------------ results
def flow_error_statistics(dicts: Sequence[dict]) -> dict:
    """What the reference's ``read_flow_error_text`` reports for the lines of ``dicts``: per key mean, rms, std, min, max and
    n_data over the frames (NaN read as 0, the N-pixel errors in percent, AE over its non-zero entries)."""
    if not dicts:
        return {}
    stats = {}
    for k in dicts[0]:
        v = np.array([0.0 if np.isnan(d[k]) else float(d[k]) for d in dicts], dtype=np.float64)
        if k in ("1PE", "2PE", "3PE", "5PE", "10PE", "20PE"):
            v = v * 100.0
        if k == "AE":
            v = v[v != 0]
        if v.size == 0:
            stats[k] = {"mean": float("nan"), "rms": float("nan"), "std": float("nan"), "min": float("nan"), "max": float("nan"),
                        "n_data": 0}
            continue
        stats[k] = {"mean": np.mean(v), "rms": np.sqrt(np.mean(np.square(v))), "std": np.std(v), "min": np.min(v), "max": np.max(v),
                    "n_data": len(v)}
    return stats


class _SaveDir(object):
    """What ``save_flow_error_as_text`` reads of a visualizer: the directory."""

    def __init__(self, save_dir: str):
        self.save_dir = save_dir


def save_line(solver, i_frame: int, d: dict, name: str, save_dir: Optional[str] = None) -> str:
    """One ``frame <i>::{...}`` line through the solver's own ``save_flow_error_as_text`` -> the file's path.  ``save_dir``, when
    given, goes before the solver's visualizer's directory: the writer takes its directory from ``solver.visualizer``, so a
    stand-in that holds only ``save_dir`` is put there for the call."""
    if save_dir is None:
        solver.save_flow_error_as_text(i_frame, d, name)
        return os.path.join(solver.visualizer.save_dir, name) if solver.visualizer is not None else name
    kept = solver.visualizer
    solver.visualizer = _SaveDir(save_dir)
    try:
        solver.save_flow_error_as_text(i_frame, d, name)
    finally:
        solver.visualizer = kept
    return os.path.join(save_dir, name)


@dataclass
class EvaluationResult(object):
    steps: List[EvalStep] = field(default_factory=list)              # the steps that were run
    skipped: List[EvalStep] = field(default_factory=list)            # the pairs the driver skips (wrong cropped shape)
    errors_without_mask: List[dict] = field(default_factory=list)
    errors_with_mask: List[dict] = field(default_factory=list)
    timestamps: List[dict] = field(default_factory=list)
    batch_time_scales: List[float] = field(default_factory=list)
    flows: Optional[list] = None           # on request: per step (estimation, reference flow) device tensors
    poisson: Optional[list] = None         # on request: per step (P of the scaled estimate, P of the reference flow) device tensors
    files: dict = field(default_factory=dict)
    pictures: Optional[list] = None        # with pictures=True: per step {name: uint8 numpy picture} as written
    photometric: Optional[list] = None             # with photometric=True: per step the photometric score of the scaled estimate ...
    photometric_reference: Optional[list] = None   # ... and of the frame-based flow ({column of photometric.COLUMNS: np.float64})

    @property
    def statistics(self) -> dict:
        return {"without_mask": flow_error_statistics(self.errors_without_mask),
                "with_mask": flow_error_statistics(self.errors_with_mask)}


# ------------------------------------------------------------------------------------------------ the evaluator
class RecordingEvaluator(object):
    """``evaluate_per_frames`` of the reference driver over a recording.

    Args:
        config ... the propagated YAML (``utils.propagate_config``): evaluation, common_params, data, method, params_opencv_flow.
        events ... ``RawEventStore``;  frames ... ``FrameStore``.
        solver ... a solver of ``solver.collections`` built for (data.height, data.width) and the crop.
        save_dir ... where the three text files go; None: the solver's visualizer's ``save_dir``, else the working directory.

    A solver without ``estimate_batch_prepared`` is driven through ``preprocess`` + ``estimate``, whose interface is numpy: that
    path downloads the reference flow and the frame of every window and uploads the estimate again.
    """

    def __init__(self, config: dict, events, frames, solver, save_dir: Optional[str] = None):
        if config.get("method") not in SUPPORTED_METHODS:
            raise NotImplementedError(f"method {config.get('method')!r} is not supported ({', '.join(SUPPORTED_METHODS)})")
        if config.get("estimation_method", "solver") != "solver":
            raise NotImplementedError(f"estimation_method {config.get('estimation_method')!r} is not supported (solver)")
        self.config, self.events, self.frames, self.solver, self.save_dir = config, events, frames, solver, save_dir
        self.common = config["common_params"]
        self.remove = NOSE_RECT if bool(config["data"].get("remove_nose", False)) else None
        self.prepared_path = hasattr(solver, "estimate_batch_prepared")
        self.flow_estimator = frame_flow.FrameFlowEstimator(None)
        self._picture_writer = None

    # ------------------------------------------------------------------ frames and the frame-based flow
    def _load_frames(self, indices: Sequence[int]):
        """Every distinct frame of ``indices`` once, warped, un-cropped -> (device [n, H, W], position of each index)."""
        distinct = sorted(set(int(i) for i in indices))
        full, _ = self.frames.load_images(distinct, roi=None)
        return full, {i: k for k, i in enumerate(distinct)}

    def _crop(self, full: torch.Tensor) -> torch.Tensor:
        c = self.common
        return full[..., c["xmin"]:c["xmax"], c["ymin"]:c["ymax"]]

    def _reference_flow(self, crop0: torch.Tensor, crops: torch.Tensor, k1: Sequence[int], k2: Sequence[int]) -> torch.Tensor:
        """The frame-based flow of the pairs (crops[k1[b]], crops[k2[b]]) -> device float32 [B, 2, Hf, Wf], padded back to the
        full frame as ``FrameFlowEstimator`` pads it."""
        return self.flow_estimator.estimate_batch(self.config["method"], crop0, crops, k1, k2, self.config)

    # ------------------------------------------------------------------ events
    def _ingest(self, steps: Sequence[EvalStep]) -> PreparedWindows:
        """The estimation windows of ``steps`` -> PreparedWindows (one launch; with BAF / HOT listed the filters run window by
        window first, as ``preprocess`` chains them)."""
        solver, store = self.solver, self.events
        H, W = (int(v) for v in solver.orig_image_shape)
        tps = store.TICKS_PER_SECOND
        for s in steps:
            store._check(*s.gt_range)    # (the driver's load_event of both batches: IndexError for an empty slice)
            store._check(*s.est_range)
        if solver.filter_set is None:
            lo, hi = min(s.est_range[0] for s in steps), max(s.est_range[1] for s in steps)
            cols = store.load_raw(lo, hi)
            ranges = [(s.est_range[0] - lo, s.est_range[1] - lo) for s in steps]
            return window_ingest_raw_batch(cols, ranges, (H, W), solver.roi, self.remove, tps)
        kept, periods, ranges, at = [], [], [], 0
        for s in steps:
            col, row, t, pol = store.load_raw(*s.est_range)
            keep = _keep_mask(col, row, None, self.remove)
            if keep is not None:
                col, row, t, pol = col[keep], row[keep], t[keep], pol[keep]
            if int(t.shape[0]) >= event_filters.MIN_EVENTS:   # preprocess: fewer events are returned as they are
                keep = _keep_mask(col, row, solver.roi, None)
                if keep is not None:
                    col, row, t, pol = col[keep], row[keep], t[keep], pol[keep]
            n = int(t.shape[0])
            periods.append((_seconds(t.max(), tps) - _seconds(t.min(), tps)) if n else torch.zeros((), dtype=torch.float64, device=t.device))
            if n >= event_filters.MIN_EVENTS:
                col, row, t, pol = solver.filter_set.filter_raw_window(col, row, t, pol, tps)
            kept.append((col, row, t, pol))
            ranges.append((at, at + int(t.shape[0])))
            at += int(t.shape[0])
        cols = tuple(torch.cat([k[j] for k in kept]) for j in range(4))
        prepared = window_ingest_raw_batch(cols, ranges, (H, W), None, None, tps)
        prepared.period = torch.stack(periods)
        return prepared

    # ------------------------------------------------------------------ output
    def _write(self, i_frame: int, d: dict, name: str) -> str:
        return save_line(self.solver, i_frame, d, name, self.save_dir)

    # ------------------------------------------------------------------ run
    def run(self, max_batch: int = 8, poisson: bool = False, keep_flows: bool = False, pictures: bool = False,
            photometric: bool = False) -> EvaluationResult:
        """``photometric``: also score, per step, the scaled estimate ``est * gt_time_scale / period`` (the scaling of the pictures)
        and the frame-based flow against the two un-cropped frames with ``photometric.photometric_error_batch`` (two calls of two
        launches per batch, ``roi`` = the ``common_params`` rectangle; the tables come back in the batch's one read-back) ->
        ``result.photometric`` / ``result.photometric_reference`` and two more text files.  Off: nothing changes.

        ``pictures``: also render the driver's ten pictures of every step (``visualizer.render_step_batch``: one more
        ``window_ingest_raw_batch`` call for the unfiltered events between the two frames, then a fixed number of launches per
        batch) and write them, ``pred_flow<i>.npy`` and ``color_wheel.png`` under ``save_dir`` (default: the solver's
        visualizer's directory, else the working directory) as the reference names them.  Needs PIL.  Off: nothing changes."""
        if int(max_batch) != max_batch or max_batch < 1:
            raise ValueError(f"max_batch {max_batch!r} < 1")
        plan = plan_evaluation(self.config, self.events, self.frames)
        result = EvaluationResult(flows=[] if keep_flows else None, poisson=[] if poisson else None, pictures=[] if pictures else None,
                                  photometric=[] if photometric else None, photometric_reference=[] if photometric else None)
        self._picture_writer = None
        if pictures:
            from .visualizer import Visualizer

            where = self.save_dir if self.save_dir is not None else getattr(self.solver.visualizer, "save_dir", "./")
            self._picture_writer = Visualizer(tuple(self.solver.orig_image_shape), save=True, save_dir=where)
        todo = []
        for s in plan:
            if s.run:
                todo.append(s)
            else:
                logger.warning(f"Warning! The frame might be collapsed -- i1 = {s.i1}, i2 = {s.i2}")
                result.skipped.append(s)
        if self.save_dir is not None:
            os.makedirs(self.save_dir, exist_ok=True)
        if not todo:
            return result
        full0 = self.frames.load_images([0], roi=None)[0][0]
        for lo in range(0, len(todo), int(max_batch)):
            self._run_batch(todo[lo:lo + int(max_batch)], full0, result, poisson)
        return result

    def _ingest_unfiltered(self, steps: Sequence[EvalStep]) -> torch.Tensor:
        """The events between the two frames of every step, un-cropped (the driver's ``batch_for_gt``, nose removed when asked)
        -> their polarity counts [B, 2, H, W], one launch."""
        lo, hi = min(s.gt_range[0] for s in steps), max(s.gt_range[1] for s in steps)
        cols = self.events.load_raw(lo, hi)
        ranges = [(s.gt_range[0] - lo, s.gt_range[1] - lo) for s in steps]
        H, W = (int(v) for v in self.solver.orig_image_shape)
        return window_ingest_raw_batch(cols, ranges, (H, W), None, self.remove, self.events.TICKS_PER_SECOND).pol

    def _draw(self, steps, est, gt, mask, filter_pol, period, result: EvaluationResult) -> None:
        """The pictures of a batch: rendered at once, read back once per picture kind, written step by step in the driver's order."""
        from .visualizer import PICTURES, color_wheel, render_step_batch

        viz, solver = self._picture_writer, self.solver
        scale = torch.tensor([s.gt_time_scale for s in steps], dtype=torch.float64, device=est.device) / period.to(est.device)
        pred = est.double() * scale[:, None, None, None]
        pics = render_step_batch(pred, gt, mask, filter_pol, self._ingest_unfiltered(steps), getattr(solver, "pad", 0),
                                 getattr(solver, "iwe_visualize_max_scale", 50))
        host = {k: v.cpu().numpy() for k, v in pics.items()}
        flows = pred.cpu().numpy()
        wheel = color_wheel(int(pred.shape[2]), pred.device).cpu().numpy()
        for b, _ in enumerate(steps):
            for name in PICTURES:
                if name == "pred_flow":
                    viz.save_array(flows[b], "pred_flow")          # (visualize_optical_flow(save_flow=True): the .npy, same number)
                viz.visualize_image(host[name][b], file_prefix=name)
                if name == "flow_comparison_gt":
                    viz._show_or_save_image(wheel, fixed_file_name="color_wheel")
                listed = getattr(solver, "sequential_video_list", None)
                if listed is not None and not name.startswith("flow_comparison") and name not in listed:
                    listed.append(name)
            result.pictures.append({name: host[name][b] for name in PICTURES})

    def _run_batch(self, steps: Sequence[EvalStep], full0: torch.Tensor, result: EvaluationResult, poisson: bool) -> None:
        c = self.common
        full, pos = self._load_frames([s.i1 for s in steps] + [s.i2 for s in steps])
        k1, k2 = [pos[s.i1] for s in steps], [pos[s.i2] for s in steps]
        gt = self._reference_flow(self._crop(full0), self._crop(full), k1, k2)
        if self.prepared_path:
            prepared = self._ingest(steps)
            est = self.solver.estimate_batch_prepared(prepared, frames=[full[k] for k in k1], background=full0,
                                                      max_batch=len(steps), device_out=True)
            mask, period, filter_pol = prepared.mask, prepared.period, prepared.pol
        else:
            est, mask, period, filter_pol = self._solve_sequential(steps, gt, full, k1, full0)
        if result.pictures is not None:
            self._draw(steps, est, gt, mask, filter_pol, period, result)
        roi = (slice(None), slice(None), slice(c["xmin"], c["xmax"]), slice(c["ymin"], c["ymax"]))
        plain, _ = flow_error.flow_error_batch(gt[roi], est[roi])
        masked, _ = flow_error.flow_error_batch(gt[roi], est[roi], event_mask=mask[roi[0], roi[2], roi[3]][:, None])
        columns = [plain[:, :8], masked[:, :8], period.reshape(-1, 1).to(plain.device)]
        if result.photometric is not None:
            columns += self._photometric(steps, full, k1, k2, est, gt, period)
        small = torch.cat(columns, dim=1).cpu().numpy()   # the batch's one read-back
        if poisson:
            from .poisson import poisson_reconstruct_batch

            scale = torch.tensor([s.gt_time_scale for s in steps], dtype=torch.float64, device=est.device) / period.to(est.device)
            p_est = poisson_reconstruct_batch(est * scale[:, None, None, None])
            p_gt = poisson_reconstruct_batch(gt)
        for b, s in enumerate(steps):
            e0 = {k: np.float64(small[b, j]) for j, k in enumerate(flow_error.KEYS)}
            e1 = {k: np.float64(small[b, 8 + j]) for j, k in enumerate(flow_error.KEYS)}
            ts = {"t1": s.t1, "t2": s.t2}
            result.files[TEXT_WITHOUT_MASK] = self._write(s.i_frame, e0, TEXT_WITHOUT_MASK)
            result.files[TEXT_WITH_MASK] = self._write(s.i_frame, e1, TEXT_WITH_MASK)
            result.files[TEXT_TIMESTAMPS] = self._write(s.i_frame, ts, TEXT_TIMESTAMPS)
            result.steps.append(s)
            result.errors_without_mask.append(e0)
            result.errors_with_mask.append(e1)
            result.timestamps.append(ts)
            result.batch_time_scales.append(float(small[b, 16]))
            if result.photometric is not None:
                n = len(photometric.COLUMNS)
                p0 = {k: np.float64(small[b, 17 + j]) for j, k in enumerate(photometric.COLUMNS)}
                p1 = {k: np.float64(small[b, 17 + n + j]) for j, k in enumerate(photometric.COLUMNS)}
                result.files[TEXT_PHOTOMETRIC] = self._write(s.i_frame, p0, TEXT_PHOTOMETRIC)
                result.files[TEXT_PHOTOMETRIC_REFERENCE] = self._write(s.i_frame, p1, TEXT_PHOTOMETRIC_REFERENCE)
                result.photometric.append(p0)
                result.photometric_reference.append(p1)
            if result.flows is not None:
                result.flows.append((est[b], gt[b]))
            if result.poisson is not None:
                result.poisson.append((p_est[b], p_gt[b]))

    def _photometric(self, steps, full, k1, k2, est, gt, period) -> List[torch.Tensor]:
        """The photometric tables [B, 7] of the scaled estimate and of the frame-based flow on the un-cropped frames of the batch."""
        c = self.common
        roi = (c["xmin"], c["xmax"], c["ymin"], c["ymax"])
        frame1, frame2 = full[k1], full[k2]
        scale = torch.tensor([s.gt_time_scale for s in steps], dtype=torch.float64, device=est.device) / period.to(est.device)
        pred = est.double() * scale[:, None, None, None]
        tables = []
        for flow in (pred, gt):
            as_flow = (lambda f: f) if frame1.dtype == torch.uint8 else (lambda f: f.to(flow.dtype))
            tables.append(photometric.photometric_error_batch(as_flow(frame1), as_flow(frame2), flow, roi=roi)[0].to(est.device))
        return tables

    def _solve_sequential(self, steps, gt, full, k1, full0):
        """A solver without a prepared path: ``preprocess`` + ``estimate`` per window, as the driver calls them."""
        from .utils import remove_event

        solver = self.solver
        im0 = full0.cpu().numpy()
        ests, masks, periods, pols = [], [], [], []
        for b, s in enumerate(steps):
            self.events._check(*s.gt_range)
            batch = self.events.load_event(*s.est_range)
            if self.remove is not None:
                batch = remove_event(batch, *self.remove)
            filtered, period = solver.preprocess(batch)
            est = solver.estimate(filtered, gt[b].cpu().numpy(), frame=full[k1[b]].cpu().numpy(), background=im0)
            ests.append(torch.as_tensor(np.asarray(est), dtype=torch.float64).to(gt.device))
            ev = torch.as_tensor(filtered, dtype=torch.float64).to(gt.device)
            masks.append(solver.orig_imager.create_eventmask(ev).reshape(tuple(solver.orig_image_shape)).to(torch.uint8))
            periods.append(float(period))
            if self._picture_writer is not None:
                pols.append(self._picture_writer.imager.create_image_from_events_tensor(ev, method="polarity", sigma=0)
                            .reshape(2, *solver.orig_image_shape))
        return (torch.stack(ests), torch.stack(masks), torch.tensor(periods, dtype=torch.float64, device=gt.device),
                torch.stack(pols) if pols else None)


# ------------------------------------------------------------------------------------------------ a synthetic recording
def synthetic_recording(directory: str, image_shape=(64, 96), n_frames: int = 8, events_per_interval: int = 4000, seed: int = 0,
                        frame_period_us: int = 10_000, hot_pixel: Optional[Tuple[int, int]] = None):
    """(For ``tools/run_eval.py --synthetic``, ``tools/bench_eval.py`` and the tests; not part of ``__all__``.)  A small recording
    in ``directory``: random-dot frames displaced by a smooth, growing bump; the events those frames imply on
    integer pixels (a brightness rise between two frames fires positive events, a fall negative ones, with times spread over the
    interval); trigger timestamps.  Returns (events .npz path, frames .npy path, trigger file path, frame timestamps in seconds).
    ``hot_pixel``: one pixel that also fires in every interval, as a stuck pixel does."""
    rs = np.random.RandomState(seed)
    H, W = (int(v) for v in image_shape)
    os.makedirs(directory, exist_ok=True)
    base = rs.rand(H + 16, W + 16)
    k = np.array([1, 4, 6, 4, 1], dtype=np.float64) / 16
    for axis in (0, 1):
        base = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), axis, base)
    base = (base - base.min()) / (base.max() - base.min())
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    bump = np.exp(-((yy - H / 2) ** 2 / (H / 4) ** 2 + (xx - W / 2) ** 2 / (W / 4) ** 2))
    frames = np.zeros((n_frames, H, W), dtype=np.uint8)
    for f in range(n_frames):
        sy, sx = yy + 8 + 0.6 * f * bump, xx + 8 + 0.4 * f * bump
        y0, x0 = np.floor(sy).astype(int), np.floor(sx).astype(int)
        fy, fx = sy - y0, sx - x0
        img = (base[y0, x0] * (1 - fy) * (1 - fx) + base[y0 + 1, x0] * fy * (1 - fx) + base[y0, x0 + 1] * (1 - fy) * fx
               + base[y0 + 1, x0 + 1] * fy * fx)
        frames[f] = np.clip(img * 255.0, 0, 255).astype(np.uint8)
    stamps = (np.arange(n_frames, dtype=np.int64) + 1) * int(frame_period_us)
    xs, ys, tsl, ps = [], [], [], []
    for f in range(n_frames - 1):
        diff = frames[f + 1].astype(np.float64) - frames[f].astype(np.float64)
        w = np.abs(diff).ravel() + 1e-3
        pick = rs.choice(H * W, size=events_per_interval, p=w / w.sum())
        if hot_pixel is not None:
            pick[: events_per_interval // 8] = hot_pixel[0] * W + hot_pixel[1]
        t = np.sort(rs.randint(stamps[f], stamps[f + 1], size=events_per_interval))
        xs.append(pick % W)
        ys.append(pick // W)
        tsl.append(t)
        ps.append(diff.ravel()[pick] >= 0)
    from .data_loader import RawEventStore

    ev_path = os.path.join(directory, "events.npz")
    RawEventStore.save(ev_path, np.concatenate(xs), np.concatenate(ys), np.concatenate(tsl), np.concatenate(ps))
    fr_path = os.path.join(directory, "frames.npy")
    np.save(fr_path, frames)
    tr_path = os.path.join(directory, "trigger_events.txt")
    with open(tr_path, "w") as f:
        for i, t in enumerate(stamps):
            f.write(f"{int(t)} 0 1\n{int(t) + 100} 0 0\n")
    return ev_path, fr_path, tr_path, stamps / 1e6


__all__ = ["EvalStep", "plan_evaluation", "PreparedWindows", "window_ingest_raw_batch", "flow_error_statistics", "EvaluationResult",
           "RecordingEvaluator", "NOSE_RECT"]
