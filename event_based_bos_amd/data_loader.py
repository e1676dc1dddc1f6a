"""Ingest for the hot path: a raw-column event store and a frame store, the two halves of the reference's
co-capture loader (src/data_loader/ccs.py, ``CcsDataLoader``).

The reference reads CCS recordings from HDF5 (``raw_events/{x: int16, y: int16, t: int32 us, p: bool}``,
src/data_loader/ccs.py:57-66) and hands every window to the solver as a float64 ``[n, 4]`` array
``(row = y, col = x, t / 1e6, p)`` (:289-297).  ``h5py`` is not part of this image, so the store keeps the same
four columns in an uncompressed ``.npz`` (keys ``raw_events_x/y/t/p``; an ``.hdf5`` path is read directly where ``h5py`` exists,
``_hdf5.py``; the camera's own ``cd_events.raw``, ccs.py:171 -- EVT 2.0, 2.1 or 3.0 -- and ``.dat`` files are decoded on the GPU,
``recordings.py``, and a ``.raw`` file brings its trigger edges along as ``store.triggers``) -- and, more to the point, it can hand a
window to the GPU *as raw columns* (9 B/event instead of 32 B/event over PCIe), where ``EventPlan.build_raw``
expands it with the same fp64 time arithmetic.

    store = RawEventStore("recording.npz")
    events = store.load_event(i0, i1)                    # reference format, for any reference-style caller
    plan = store.plan(i0, i1, (720, 1280), "first")      # fast path: raw columns -> device -> EventPlan

With ``calibration=`` (a ``calibration.CameraCalibration``, or the ``{"K", "D"}`` dict ``load_calib`` returns) the store answers the
reference loaders' ``load_calib`` / ``undistort`` and hands out rectified sub-pixel windows: ``load_event(.., rectify=True)``,
``plan(.., rectify=True)``.

Index helpers follow the reference loader: ``index_to_time`` (:319-330), ``time_to_index`` = searchsorted - 1 (:343-356).

``FrameStore`` is the frame half (:36-47, :136-156, :332-343, :359-396): the camera frames, their trigger timestamps and the
homography that maps them into the event view, under the reference's method names.  ``load_image`` returns what the reference
returns; ``load_images`` uploads a batch of raw frames once and warps and crops them in one launch (frame_warp).

    frames = FrameStore("frames.npy", "trigger_events.txt", "homography.txt", (720, 1280))
    i = frames.time_to_image_index(t)
    batch, ts = frames.load_images(range(i, i + 8), roi=config["common_params"])      # device [8, h, w]
"""
from __future__ import annotations

import logging
import os
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip
from .event_plan import EventPlan
from .event_voxel import event_voxel_batch

logger = logging.getLogger(__name__)

COLUMNS = (("x", np.int16), ("y", np.int16), ("t", np.int32), ("p", np.bool_))


def _as_calibration(calibration, sensor_size):
    """None, a ``CameraCalibration``, or the {"K", "D"[, "new_K"]} dict ``load_calib`` returns (then ``sensor_size`` is required)."""
    if calibration is None:
        return None
    from .calibration import CameraCalibration

    if isinstance(calibration, CameraCalibration):
        return calibration
    if isinstance(calibration, dict):
        if calibration.get("K") is not None and calibration.get("D") is not None and sensor_size is None \
                and calibration.get("sensor_size") is None:
            raise ValueError("sensor_size (height, width) is required with a calibration given as a dict")
        return CameraCalibration.from_dict(calibration, sensor_size)
    raise ValueError(f"calibration must be a CameraCalibration or a dict with K and D, got {type(calibration).__name__}")


class RawEventStore(object):
    NAME = "RAW_COLUMNS"
    TICKS_PER_SECOND = 1e6  # microsecond timestamps, src/data_loader/ccs.py:295

    def __init__(self, source: Union[str, Dict[str, np.ndarray]], sensor_size: Optional[Tuple[int, int]] = None, calibration=None,
                 half_swapped: Optional[bool] = None):
        self.calibration = _as_calibration(calibration, sensor_size)   # None: no calibration, as the reference's loaders answer
        self.header = None            # a .raw / .dat source: the parsed header (recordings.RawHeader)
        self.triggers = None          # a .raw / .dat source: int64 [n, 3] = (t, id, value), the "old" layout of read_trigger_timestamps
        self.dropped_outside = 0      # a .raw / .dat source: events outside the header's geometry, removed
        if isinstance(source, dict):
            data = source
        elif str(source).lower().endswith((".raw", ".dat")):   # the camera's own recording, decoded on the GPU (recordings.py)
            data = self._read_raw(str(source), sensor_size, half_swapped)
        elif str(source).lower().endswith((".hdf5", ".h5")):   # the reference's own recordings, read as its h5py_loader does (needs h5py)
            from ._hdf5 import read_raw_events

            data = read_raw_events(str(source), wide_time=True)
        else:
            with np.load(source) as f:
                data = {k: f["raw_events_" + k] for k, _ in COLUMNS}
        self.event_data = {}
        for k, dt in COLUMNS:
            col = np.asarray(data[k])
            if k == "t" and col.dtype == np.int64:
                pass  # recordings beyond 2^31 us keep 64-bit ticks (the reference only warns, :60-62)
            else:
                col = col.astype(dt, copy=False)
            self.event_data[k] = np.ascontiguousarray(col)
        n = len(self.event_data["t"])
        if any(len(v) != n or v.ndim != 1 for v in self.event_data.values()):
            raise ValueError("raw event columns must be 1-D and of equal length")
        self._time_cache = None
        self._pinned = None

    def _read_raw(self, path: str, sensor_size: Optional[Tuple[int, int]], half_swapped: Optional[bool] = None) -> Dict[str, np.ndarray]:
        """The columns of a Prophesee ``.raw`` (EVT 2.0, 2.1, 3.0) or ``.dat`` file (``recordings.decode_recording``: decoded on the
        GPU), narrowed as ``save`` narrows them; the trigger edges of the same pass go to ``self.triggers`` (none in a DAT file).
        ``half_swapped``: the word order of an EVT 2.1 file, None = what its header says.  Events outside the geometry are removed
        here, on the host: the downstream kernels index by pixel."""
        from .recordings import decode_recording

        x, y, t, p, self.triggers, self.header = decode_recording(path, sensor_size=sensor_size, half_swapped=half_swapped)
        outside = (x.view(np.uint16) >= self.header.width) | (y.view(np.uint16) >= self.header.height)
        self.dropped_outside = int(outside.sum())
        if self.dropped_outside:
            logger.warning(f"{path}: {self.dropped_outside} events outside the {self.header.width} x {self.header.height} geometry removed")
            x, y, t, p = (c[~outside] for c in (x, y, t, p))
        backwards = int((np.diff(t) < 0).sum()) if len(t) > 1 else 0
        if backwards:
            logger.warning(f"{path}: t steps backwards {backwards} times; time_to_index assumes ordered timestamps")
        if not t.size or t.max() <= np.iinfo(np.int32).max:
            t = t.astype(np.int32)
        return {"x": x, "y": y, "t": t, "p": p.astype(np.bool_)}

    @staticmethod
    def save(path: str, x, y, t, p) -> None:
        """Write the four raw columns (sensor x = column, sensor y = row, t in microseconds, polarity)."""
        t = np.asarray(t)
        np.savez(path, raw_events_x=np.asarray(x, dtype=np.int16), raw_events_y=np.asarray(y, dtype=np.int16),
                 raw_events_t=t.astype(np.int64 if t.size and np.abs(t).max() > np.iinfo(np.int32).max else np.int32),
                 raw_events_p=np.asarray(p, dtype=np.bool_))

    def __len__(self) -> int:
        return len(self.event_data["x"])

    # (what set_sequence leaves on the reference's loader, src/data_loader/ccs.py:213-217)
    @property
    def min_ts(self) -> float:
        return self.event_data["t"].min() / self.TICKS_PER_SECOND

    @property
    def max_ts(self) -> float:
        return self.event_data["t"].max() / self.TICKS_PER_SECOND

    @property
    def data_duration(self) -> float:
        return self.max_ts - self.min_ts

    # ------------------------------------------------------------------ reference-format window
    def _check(self, start_index: int, end_index: int) -> None:
        if end_index > len(self):
            e = f"Specified {start_index} to {end_index} index, but there are only {len(self)} events."
            logger.error(e)
            raise IndexError(e)
        if end_index - start_index <= 0 or start_index >= len(self):
            e = f"Specified {start_index} to {end_index} index, but no events."
            logger.error(e)
            raise IndexError(e)

    def load_event(self, start_index: int, end_index: int, *args, rectify: bool = False, **kwargs) -> np.ndarray:
        """float64 [n, 4] = (row, col, t in seconds, p), as src/data_loader/ccs.py:247-297.  ``rectify=True`` (needs a calibration
        and a GPU): the window's events at their rectified sub-pixel positions, ``calibration.rectify_events_raw`` -- events that
        leave the sensor's image are dropped, so the array may be shorter; ``t`` and ``p`` are unchanged bit for bit."""
        self._check(start_index, end_index)
        if rectify:
            return self._rectified(start_index, end_index, "cuda").cpu().numpy()
        n = end_index - start_index
        events = np.zeros((n, 4), dtype=np.float64)
        sl = slice(start_index, end_index)
        events[:, 0] = self.event_data["y"][sl]
        events[:, 1] = self.event_data["x"][sl]
        events[:, 2] = self.event_data["t"][sl] / self.TICKS_PER_SECOND
        events[:, 3] = self.event_data["p"][sl]
        return events

    # ------------------------------------------------------------------ raw window on the device
    def pin(self) -> "RawEventStore":
        """Page-lock the four columns once (9 B/event of host memory): every later window upload is then a plain
        asynchronous DMA from the recording itself -- no per-window staging buffer, no pinned allocation (tens of
        milliseconds each) on the ingest path."""
        if not self._pinned:
            _hip.require_gpu()
            self._pinned = {k: torch.from_numpy(self.event_data[k].view(np.uint8) if k == "p" else self.event_data[k]).pin_memory()
                            for k in ("x", "y", "t", "p")}
        return self

    def load_raw(self, start_index: int, end_index: int, device="cuda") -> Tuple[torch.Tensor, ...]:
        """(col int16, row int16, t int32|int64, pol uint8) of the window on ``device``: asynchronous copies on the
        current stream straight from the page-locked columns (9 B/event)."""
        self._check(start_index, end_index)
        dev = torch.device(device)
        if self._pinned is None:
            try:
                self.pin()
            except RuntimeError as err:  # recording too large to page-lock whole: stage window by window instead
                logger.warning(f"could not page-lock the recording ({err}); staging every window separately")
                self._pinned = False
        if self._pinned:
            return tuple(self._pinned[k][start_index:end_index].to(dev, non_blocking=True) for k in ("x", "y", "t", "p"))
        sl = slice(start_index, end_index)
        cols = (torch.from_numpy(self.event_data[k][sl].view(np.uint8) if k == "p" else self.event_data[k][sl]) for k in "xytp")
        return tuple(c.pin_memory().to(dev, non_blocking=True) for c in cols)

    # ------------------------------------------------------------------ calibration (reference: ccs.py:427-451)
    def load_calib(self) -> dict:
        """{"K": camera matrix, "D": distortion coefficients}; both None without a calibration, as the reference's loaders answer."""
        if self.calibration is None:
            return {"K": None, "D": None}
        return self.calibration.as_dict()

    def undistort(self, event_batch):
        """``utils.undistort_events`` with the store's own rectification map (integer positions, the reference's semantics).
        Without a calibration: ``NotImplementedError``, as the reference's loaders raise."""
        if self.calibration is None:
            logger.error("Not supported!")
            raise NotImplementedError("the store has no calibration: pass calibration= (a CameraCalibration or a {'K', 'D'} dict)")
        from .calibration import undistort_events

        dev = event_batch.device if isinstance(event_batch, torch.Tensor) and event_batch.is_cuda else None
        rmap = self.calibration.rectify_map(dev)
        H, W = self.calibration.sensor_size
        return undistort_events(event_batch, rmap[..., 1], rmap[..., 0], H, W)

    def _rectified(self, start_index: int, end_index: int, device, dtype=torch.float64) -> torch.Tensor:
        if self.calibration is None:
            raise ValueError("rectify=True needs a calibration: pass calibration= (a CameraCalibration or a {'K', 'D'} dict)")
        from .calibration import rectify_events_raw

        _hip.require_gpu()
        col, row, t, pol = self.load_raw(start_index, end_index, device)
        events, outside_sensor, outside_image = rectify_events_raw(col, row, t, pol, self.calibration, self.TICKS_PER_SECOND, dtype)
        if outside_sensor or outside_image:
            logger.info(f"events {start_index} .. {end_index}: {outside_sensor} outside the sensor, {outside_image} rectified to outside "
                        "the image, dropped")
        return events

    def plan(self, start_index: int, end_index: int, image_size: Tuple[int, int], direction="first",
             normalize_t: bool = True, tile="auto", device="cuda", deferred: bool = False, emit: str = "full",
             rectify: bool = False) -> EventPlan:
        """``rectify=True``: ``EventPlan.build`` -- the full build, which is what fractional windows take -- on the window's rectified
        events (``calibration.rectify_events_raw``); ``deferred`` and ``emit`` other than "full" are refused."""
        if rectify:
            if deferred or emit != "full":
                raise ValueError("rectify=True takes the full plan build: the lean and deferred builds are integer-only")
            self._check(start_index, end_index)
            return EventPlan.build(self._rectified(start_index, end_index, device), image_size, direction, normalize_t, tile)
        col, row, t, pol = self.load_raw(start_index, end_index, device)
        return EventPlan.build_raw(col, row, t, pol, image_size, direction, normalize_t, tile, self.TICKS_PER_SECOND,
                                   deferred=deferred, emit=emit)

    def plans(self, windows, image_size: Tuple[int, int], direction="first", normalize_t: bool = True, tile="auto", device="cuda",
              deferred: bool = True) -> list:
        """The lean plans of several (start_index, end_index) windows in one set of launches: the batched sibling of ``plan(...,
        emit="compact")``, ``EventPlan.build_raw_batch``.  The stretch of the recording from the first window's start to the last
        one's end is uploaded ONCE (windows of a recording follow or overlap each other; events between far-apart windows travel
        along), and every window is a range of it.  Plan k equals ``plan(*windows[k], ..., emit="compact")`` bit for bit."""
        windows = [(int(a), int(b)) for a, b in windows]
        if not windows:
            return []
        for a, b in windows:
            self._check(a, b)
        lo, hi = min(a for a, _ in windows), max(b for _, b in windows)
        col, row, t, pol = self.load_raw(lo, hi, device)
        return EventPlan.build_raw_batch(col, row, t, pol, [(a - lo, b - lo) for a, b in windows], image_size, direction, normalize_t,
                                         tile, self.TICKS_PER_SECOND, deferred=deferred)

    def voxels(self, ranges, n_bins: int, image_size: Tuple[int, int], roi=None, signed: bool = True, normalize: bool = False,
               device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
        """The event voxel grids (``create_event_voxel``) of several (start_index, end_index) windows in one set of launches:
        ``event_voxel.event_voxel_batch`` with the sensor column as x and the row as y, so a plane of a grid is an image.  As in
        ``plans``, the stretch of the recording the windows cover is uploaded once.  Returns (grids float64 [B, n_bins, H, W] -- the
        ``roi`` crop with one --, valid int32 [B]); unlike ``load_event``, an empty window is allowed: its grid is zero, its
        ``valid`` 0."""
        windows = [(int(a), int(b)) for a, b in ranges]
        n = len(self)
        for a, b in windows:
            if not 0 <= a <= n or not 0 <= b <= n:
                raise IndexError(f"Specified {a} to {b} index, but there are only {n} events.")
        windows = [(a, max(a, b)) for a, b in windows]
        if not windows:
            raise ValueError("ranges holds no window")
        lo, hi = min(a for a, _ in windows), max(b for _, b in windows)
        if hi > lo:
            cols = self.load_raw(lo, hi, device)
        else:   # nothing but empty windows: no event to upload
            cols = tuple(torch.empty(0, dtype=d, device=device) for d in (torch.int16, torch.int16, torch.int32, torch.uint8))
        return event_voxel_batch(cols, [(a - lo, b - lo) for a, b in windows], n_bins, image_size, roi, signed, normalize,
                                 self.TICKS_PER_SECOND)

    # ------------------------------------------------------------------ index <-> time
    def _times(self) -> np.ndarray:
        if self._time_cache is None:
            self._time_cache = self.event_data["t"] / self.TICKS_PER_SECOND
        return self._time_cache

    def index_to_time(self, index: int) -> float:
        return self._times()[index]

    def time_to_index(self, time: float) -> int:
        return int(np.searchsorted(self._times(), time)) - 1


# file name suffixes that count as camera frames in a frame directory (the set the reference's loader accepts)
_FRAME_SUFFIXES = frozenset((".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp", ".dng", ".mpo"))


def list_frame_files(directory: str) -> list:
    """The frame files of ``directory`` in name order: regular entries whose suffix, in any letter case, is an image suffix."""
    names = sorted(n for n in os.listdir(directory) if os.path.splitext(n)[1].lower() in _FRAME_SUFFIXES)
    return [os.path.join(directory, n) for n in names]


def _trigger_rows(path: str):
    """The integer records of a trigger text file and their column layout: "old" = whitespace-separated (t, id, polarity),
    "new" = comma-separated (polarity, id, t).  The separator of the first record decides."""
    with open(path) as f:
        lines = [ln for ln in (raw.strip() for raw in f) if ln and not ln.startswith("#")]
    if not lines:
        raise ValueError(f"{path} holds no trigger records")
    comma = "," in lines[0]
    if comma:
        logger.info(f"{path}: comma-separated trigger records (polarity, id, t)")
    try:
        rows = np.array([[int(v) for v in (ln.split(",") if comma else ln.split())] for ln in lines], dtype=np.int64)
    except ValueError as err:
        raise ValueError(f"{path}: trigger records must be three integers a line ({err})") from None
    return rows, "new" if comma else "old"


def read_trigger_timestamps(source, layout: str = "auto") -> np.ndarray:
    """Trigger records -> the integer microsecond stamps of the POSITIVE edges (what the reference's loader keeps of its
    ``trigger_events.txt``).

    A path is a text file of three integers a line in either of the two layouts the reference reads: whitespace-separated
    (t, id, polarity) or comma-separated (polarity, id, t).  An [n, 3] integer array is taken in the layout ``layout`` names
    ("old" or "new"; "auto" = "old"); a 1-D integer array holds the positive edges' stamps already."""
    if layout not in ("auto", "old", "new"):
        raise ValueError(f"layout must be 'auto', 'old' or 'new', got {layout!r}")
    if isinstance(source, (str, os.PathLike)):
        rows, found = _trigger_rows(str(source))
        if layout not in ("auto", found):
            raise ValueError(f"{source} is in the {found!r} layout, not {layout!r}")
        layout = found
    else:
        rows = np.asarray(source)
        if not np.issubdtype(rows.dtype, np.integer):
            raise ValueError(f"trigger records must be integers (microseconds), got {rows.dtype}")
        if rows.ndim == 1:
            return rows
        layout = "old" if layout == "auto" else layout
    if rows.ndim != 2 or rows.shape[1] != 3:
        raise ValueError(f"trigger records must be [n, 3], got {rows.shape}")
    t_col, p_col = (0, 2) if layout == "old" else (2, 0)
    return rows[rows[:, p_col] == 1, t_col]


def _read_image(path: str) -> np.ndarray:
    """A frame file as a grey uint8 [Hs, Ws] array (what ``cv2.imread(path, IMREAD_GRAYSCALE)`` hands the reference's loader; a
    colour file goes through PIL's own luma conversion)."""
    try:
        from PIL import Image
    except ImportError as err:
        raise ImportError("reading frame files needs PIL (Pillow); pass the frames as an [N, Hs, Ws] array or .npy instead") from err
    with Image.open(path) as im:
        return np.asarray(im.convert("L"), dtype=np.uint8)


class FrameStore(object):
    """The frame half of ``CcsDataLoader``.

    Args:
        frames ... an [N, Hs, Ws] uint8 / float32 array, a ``.npy`` / ``.npz`` path holding one (``.npz``: key ``frames``, or its
            only array), or a directory of image files (sorted; the reference's suffix list; read with PIL).
        timestamps ... the trigger file (either text format) or an array, see ``read_trigger_timestamps``; seconds = stamps / 1e6.
        homography ... None (frames are returned as they are), a text file (``np.loadtxt``) or a 3 x 3 array: camera -> event view.
        sensor_size ... (height, width) of the event sensor: the size warped frames have.  Required with a homography.
        calibration ... None, or the ``CameraCalibration`` of the FRAME camera (its ``sensor_size`` is the raw frames' size): frames
            are then rectified, and warped where a homography (rectified frame -> event view) is set, in one resample
            (``frame_warp.undistort_image``).  Without one nothing changes.
    """
    def __init__(self, frames, timestamps, homography=None, sensor_size: Optional[Tuple[int, int]] = None,
                 timestamp_layout: str = "auto", calibration=None):
        if calibration is not None and not hasattr(calibration, "camera_array"):
            raise ValueError("calibration must be a CameraCalibration of the frame camera (its sensor_size is the raw frames' size)")
        self.calibration = calibration
        self._files, self._stack = None, None
        if isinstance(frames, (str, os.PathLike)):
            frames = str(frames)
            if os.path.isdir(frames):
                self._files = list_frame_files(frames)
            elif frames.lower().endswith(".npz"):
                with np.load(frames) as f:
                    keys = list(f.keys())
                    if "frames" not in keys and len(keys) != 1:
                        raise ValueError(f"{frames} holds {keys}: expected the key 'frames' or a single array")
                    self._stack = f["frames" if "frames" in keys else keys[0]]
            elif frames.lower().endswith(".npy"):
                self._stack = np.load(frames)
            else:
                raise ValueError(f"{frames} is neither a directory of image files nor a .npy / .npz stack")
        elif isinstance(frames, np.ndarray):
            self._stack = frames
        else:
            raise ValueError(f"frames must be an [N, Hs, Ws] array, a .npy / .npz path or a directory, got {type(frames).__name__}")
        if self._stack is not None:
            if self._stack.ndim != 3 or self._stack.dtype not in (np.uint8, np.float32):
                raise ValueError(f"the frame stack must be [N, Hs, Ws] uint8 or float32, got {self._stack.shape} {self._stack.dtype}")
            self._stack = np.ascontiguousarray(self._stack)
        self.timestamps = read_trigger_timestamps(timestamps, timestamp_layout) / 1e6
        self.homography = None
        if homography is not None:
            h = np.loadtxt(homography) if isinstance(homography, (str, os.PathLike)) else np.asarray(homography, dtype=np.float64)
            if h.shape != (3, 3) or not np.isfinite(h).all():
                raise ValueError(f"the homography must be a finite 3 x 3 matrix, got shape {h.shape}")
            if sensor_size is None:
                raise ValueError("sensor_size (height, width) is required with a homography")
            self.homography = np.ascontiguousarray(h, dtype=np.float64)
        self._HEIGHT, self._WIDTH = (None, None) if sensor_size is None else (int(sensor_size[0]), int(sensor_size[1]))
        if sensor_size is not None and (self._HEIGHT < 1 or self._WIDTH < 1):
            raise ValueError(f"sensor_size must be positive, got {sensor_size}")
        self._pinned = None

    @property
    def warp_frame(self) -> bool:
        return self.homography is not None

    @property
    def num_images(self) -> int:
        return len(self._files) if self._stack is None else len(self._stack)

    def image_index_to_time(self, index: int) -> float:
        return self.timestamps[index]

    def time_to_image_index(self, time: float) -> int:
        return int(np.searchsorted(self.timestamps, time)) - 1

    # ------------------------------------------------------------------ frames
    def _raw(self, index: int) -> np.ndarray:
        return self._stack[index] if self._stack is not None else _read_image(self._files[index])

    def _check_index(self, index) -> int:
        """0 .. num_images - 1.  Stricter than the reference, whose ``load_image`` only asserts ``index < len`` and so takes -1 for
        the last frame: ``time_to_image_index`` answers -1 for a time before the first frame, and loading the LAST frame for it
        would be a silent error.  (``image_index_to_time`` indexes the timestamps as the reference does, negative indices included.)"""
        if int(index) != index or not 0 <= index < self.num_images:
            raise IndexError(f"image index {index} outside 0 .. {self.num_images - 1}")
        return int(index)

    def image_shape(self, index: int) -> Tuple[int, int]:
        """(rows, columns) of what ``load_image(index)`` returns, without warping anything."""
        index = self._check_index(index)
        if self.warp_frame:
            return self._HEIGHT, self._WIDTH
        if self._stack is not None:
            return tuple(int(v) for v in self._stack.shape[1:])
        return tuple(int(v) for v in self._raw(index).shape)

    def load_image(self, index: int) -> Tuple[np.ndarray, float]:
        """(image, timestamp) as src/data_loader/ccs.py:373-396: the frame, warped to the sensor's (height, width) where a
        homography is set (that runs on the GPU), as a numpy array."""
        from . import frame_warp

        index = self._check_index(index)
        image, timestamp = self._raw(index), self.timestamps[index]
        if self.calibration is not None:
            image = frame_warp.undistort_image(image, self.calibration, self.homography,
                                               (self._WIDTH, self._HEIGHT) if self.warp_frame else None)
        elif self.warp_frame:
            image = frame_warp.warp_perspective(image, self.homography, (self._WIDTH, self._HEIGHT))
        return image, timestamp

    def pin(self) -> "FrameStore":
        """Hold every raw frame in one page-locked stack (a directory is read once): later batches upload as plain asynchronous
        copies from it."""
        if self._pinned is None:
            _hip.require_gpu()
            if self._stack is None:
                self._stack = np.stack([_read_image(f) for f in self._files])
            self._pinned = torch.from_numpy(self._stack).pin_memory()
        return self

    def load_images(self, indices: Sequence[int], roi=None, device="cuda") -> Tuple[torch.Tensor, np.ndarray]:
        """(device [B, h, w], timestamps [B]): the raw frames uploaded once, then warped and cropped by ONE launch; no host
        synchronisation.  ``roi``: the driver's ``common_params`` (dict with xmin, xmax = rows and ymin, ymax = columns) or that
        4-tuple; frame b equals ``validate_image(load_image(indices[b])[0], roi)``, and like ``validate_image`` a ``roi`` with an odd
        number of rows or columns raises ``AssertionError``."""
        from . import frame_warp

        idx = [self._check_index(i) for i in indices]
        if not idx:
            raise ValueError("indices holds no frame")
        first = self._raw(idx[0])
        H, W = (self._HEIGHT, self._WIDTH) if self.warp_frame else first.shape
        rect = frame_warp._check_roi(roi, H, W)
        if roi is not None:
            frame_warp.check_even_crop(rect[1] - rect[0], rect[3] - rect[2], rect)
        _hip.require_gpu()
        dev = torch.device(device)
        contiguous = idx == list(range(idx[0], idx[0] + len(idx)))
        if self._pinned is not None:
            host = self._pinned[idx[0]:idx[0] + len(idx)] if contiguous else self._pinned[torch.as_tensor(idx)].pin_memory()
        elif self._stack is not None:
            host = torch.from_numpy(self._stack[idx[0]:idx[0] + len(idx)] if contiguous else self._stack[idx])
        else:
            host = torch.from_numpy(np.stack([first] + [self._raw(i) for i in idx[1:]]))
        raw = host.to(dev, non_blocking=True)
        ts = self.timestamps[idx]
        if self.calibration is not None:
            return frame_warp.undistort_image_batch(raw, self.calibration, self.homography, (W, H) if self.warp_frame else None,
                                                    roi=rect), ts
        if not self.warp_frame:
            return raw[:, rect[0]:rect[1], rect[2]:rect[3]], ts
        return frame_warp.warp_perspective_batch(raw, self.homography, (W, H), roi=rect), ts


collections = {RawEventStore.NAME: RawEventStore}
