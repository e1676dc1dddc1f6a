"""Prophesee recordings in every format the cameras and tools write: EVT 2.0, EVT 2.1 and EVT 3.0 ``.raw`` files and ``.dat``
files.  The headers and the encoders are host code (numpy); the decode runs on the GPU (csrc/evt2.hip; EVT 3.0: ``evt3.py``).

    x, y, t, p, triggers, header = decode_recording("cd_events.raw")    # any of the four; host columns, triggers [n, 3] = (t, id, value)
    slab = decode_evt2(words)                       # one slab of uint32 words -> device columns + the carry
    slab = decode_evt21(words, half_swapped=False)  # one slab of uint64 words
    x, y, t, p = decode_dat(records, version=2)     # uint32 [n, 2] = (ts, data) -> device columns

The word rules are those of include/ebos_hip.h.  There is no CPU decode: without a GPU every ``decode_*`` raises
``HipUnavailableError``.  ``encode_evt2`` / ``encode_evt21`` / ``encode_dat``, ``write_raw_file`` and ``write_dat_file`` write
streams and files for tests, tools and synthetic recordings.

Neither OpenEB nor a camera file was at hand.  The rules are written from the format documentation, and the decoder is checked
against a restatement of these rules, not against OpenEB.  The EVT 2.1 header rule stands on the same footing: a format line that
holds ``endianness=little`` means plain 64-bit words; ``% evt 2.1`` alone, or a format line without that option, means the legacy
order with the two 32-bit halves of every word exchanged (``half_swapped``); a ``half_swapped=`` argument overrides both.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from collections import namedtuple
from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip, evt3
from .evt3 import RawHeader

logger = logging.getLogger(__name__)

TIME_HIGH, CD_OFF, CD_ON, EXT_TRIGGER = 0x8, 0x0, 0x1, 0xA
_TH_MASK = (1 << 28) - 1
WORD_BYTES = {"EVT2": 4, "EVT21": 8}
FORMATS = ("EVT2", "EVT21", "EVT3", "DAT")

Evt2Slab = namedtuple("Evt2Slab", "x y t p trigger_t trigger_value trigger_id carry")


# ---------------------------------------------------------------------------------------------------- encoders (host)
def _columns(x, y, t, p):
    x, y, p = (np.asarray(a).astype(np.int64).ravel() for a in (x, y, p))
    t = np.asarray(t).astype(np.int64).ravel()
    if not (len(x) == len(y) == len(p) == len(t)):
        raise ValueError("x, y, t, p must be of equal length")
    if len(t) and (t[0] < 0 or np.any(np.diff(t) < 0)):
        raise ValueError("t must be non-negative and non-decreasing")
    return x, y, t, (p != 0).astype(np.int64)


def _trigger_rows(triggers):
    trig = np.zeros((0, 3), np.int64) if triggers is None else np.asarray(triggers, dtype=np.int64).reshape(-1, 3)
    if len(trig) and (trig[:, 1].min() < 0 or trig[:, 1].max() > 31):
        raise ValueError("EVT2 trigger ids are 5 bits")
    if len(trig) and (trig[0, 0] < 0 or np.any(np.diff(trig[:, 0]) < 0)):
        raise ValueError("trigger t must be non-negative and non-decreasing")
    return trig


def _merge(t, trig):
    """The merged items: trigger j sits after the events with t <= its time.  (is_trig [total], item time [total])"""
    n, m = len(t), len(trig)
    trig_pos = np.searchsorted(t, trig[:, 0], side="right") + np.arange(m)
    is_trig = np.zeros(n + m, bool)
    is_trig[trig_pos] = True
    it = np.empty(n + m, np.int64)
    it[is_trig], it[~is_trig] = trig[:, 0], t
    return is_trig, it


def _with_time_high(it, main, th_shift):
    """``main`` (one word per item, uint64) with the TIME_HIGH words in front of the items that need them: before the first item
    and on every change of ``it >> 6``, and for every wrap of the 34-bit time between two items (from 0 before the first) the pair
    TIME_HIGH(2^28 - 1), TIME_HIGH(0), which the decoder counts as one loop."""
    if len(it) == 0:
        return np.zeros(0, np.uint64)
    high = it >> 6
    loop, th = high >> 28, high & _TH_MASK
    changed = np.concatenate(([True], high[1:] != high[:-1]))
    d = loop - np.concatenate(([0], loop[:-1]))
    n_th = 2 * d + changed
    offs = np.concatenate(([0], np.cumsum(n_th + 1)))
    out = np.zeros(int(offs[-1]), np.uint64)
    at = offs[1:] - 1
    out[at] = main
    code = np.uint64(TIME_HIGH) << np.uint64(th_shift + 28)
    out[at[changed] - 1] = code | (th[changed].astype(np.uint64) << np.uint64(th_shift))
    owner = np.repeat(np.arange(len(it)), 2 * d)
    k = np.arange(len(owner)) - np.repeat(np.cumsum(2 * d) - 2 * d, 2 * d)
    out[offs[owner] + k] = code | (np.where(k % 2 == 0, _TH_MASK, 0).astype(np.uint64) << np.uint64(th_shift))
    return out


def encode_evt2(x, y, t, p, triggers=None) -> np.ndarray:
    """The events (sensor x, y < 2048, t in microseconds and non-decreasing, polarity) and ``triggers`` (int [m, 3] = (t, id, value),
    t non-decreasing, id < 32) as EVT 2.0 words (uint32): a trigger goes after the events up to its time; a TIME_HIGH comes before
    the first item and on every change of ``t >> 6``; every wrap of the 34-bit time is the pair TIME_HIGH(2^28 - 1), TIME_HIGH(0)."""
    x, y, t, p = _columns(x, y, t, p)
    trig = _trigger_rows(triggers)
    if len(t) and (x.min() < 0 or x.max() > 0x7FF or y.min() < 0 or y.max() > 0x7FF):
        raise ValueError("EVT2 addresses are 11 bits: 0 <= x, y < 2048")
    is_trig, it = _merge(t, trig)
    main = np.zeros(len(it), np.int64)
    main[is_trig] = (EXT_TRIGGER << 28) | (trig[:, 1] << 8) | (trig[:, 2] & 1)
    main[~is_trig] = (p << 28) | (x << 11) | y
    main |= (it & 0x3F) << 22
    return _with_time_high(it, main.astype(np.uint64), 0).astype(np.uint32)


def encode_evt21(x, y, t, p, triggers=None, vectorize: bool = True) -> np.ndarray:
    """The same as EVT 2.1 words (uint64, plain order).  ``vectorize``: a run of consecutive events of equal (t, y, p) whose x
    ascend inside one 32-aligned block becomes one word of base ``x & ~31``; otherwise every event is a word of base x, mask 1."""
    x, y, t, p = _columns(x, y, t, p)
    trig = _trigger_rows(triggers)
    n = len(t)
    if n and (x.min() < 0 or x.max() > 0x7FF or y.min() < 0 or y.max() > 0x7FF):
        raise ValueError("EVT2.1 addresses are 11 bits: 0 <= x, y < 2048")
    is_trig, it = _merge(t, trig)
    ev_pos = np.nonzero(~is_trig)[0]
    if n and vectorize:
        cont = np.zeros(n, bool)
        cont[1:] = ((t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & ((x[1:] >> 5) == (x[:-1] >> 5)) & (x[1:] > x[:-1]) &
                    (ev_pos[1:] == ev_pos[:-1] + 1))
        first = np.nonzero(~cont)[0]
        group = np.cumsum(~cont) - 1
        mask = np.zeros(len(first), np.int64)
        np.add.at(mask, group, np.int64(1) << (x & 31))
        base = x[first] & ~np.int64(31)
    else:
        first, mask, base = np.arange(n), np.ones(n, np.int64), x
    keep = is_trig.copy()
    keep[ev_pos[first]] = True          # an item: a trigger or the first event of a word
    main = np.zeros(len(it), np.uint64)
    u = lambda a: np.asarray(a).astype(np.uint64)  # noqa: E731
    main[is_trig] = (np.uint64(EXT_TRIGGER) << np.uint64(60)) | u(trig[:, 1] << 40) | u((trig[:, 2] & 1) << 32)
    main[ev_pos[first]] = u((p[first] << 60) | (base << 43) | (y[first] << 32) | mask)
    main |= u((it & 0x3F) << 54)
    return _with_time_high(it[keep], main[keep], 32)


def encode_dat(x, y, t, p, version: int = 2) -> np.ndarray:
    """The events as DAT records, uint32 [n, 2] = (ts, data): version 2 holds 14-bit addresses, version 1 x < 512 and y < 256; t
    must fit 32 bits."""
    x, y, t, p = _columns(x, y, t, p)
    if version not in (1, 2):
        raise ValueError(f"DAT version must be 1 or 2, got {version}")
    xbits, ybits, pshift = (9, 8, 17) if version == 1 else (14, 14, 28)
    if len(t) and (x.min() < 0 or x.max() >> xbits or y.min() < 0 or y.max() >> ybits):
        raise ValueError(f"DAT version {version} addresses: 0 <= x < {1 << xbits}, 0 <= y < {1 << ybits}")
    if len(t) and t[-1] >> 32:
        raise ValueError("DAT times are 32 bits")
    return np.stack([t, x | (y << xbits) | (p << pshift)], 1).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------- files
def write_raw_file(path: str, words, width: int, height: int, fmt: str = "EVT3") -> None:
    """A ``.raw`` file of ``words`` under the header current cameras write for ``fmt`` ("EVT2": uint32, "EVT21": uint64 in plain
    order, declared by ``endianness=little``, "EVT3": uint16)."""
    fmt = fmt.upper()
    if fmt == "EVT3":
        return evt3.write_raw_file(path, words, width, height)
    if fmt not in WORD_BYTES:
        raise ValueError(f"write_raw_file writes EVT2, EVT21 and EVT3, not {fmt}")
    version, option = ("2.0", "") if fmt == "EVT2" else ("2.1", "endianness=little;")
    words = np.ascontiguousarray(np.asarray(words, dtype="<u4" if fmt == "EVT2" else "<u8"))
    with open(path, "wb") as f:
        f.write(f"% camera_integrator_name Prophesee\n% evt {version}\n% format {fmt};{option}height={int(height)};width={int(width)}\n"
                f"% geometry {int(width)}x{int(height)}\n% end\n".encode("ascii"))
        f.write(words.tobytes())


def write_dat_file(path: str, records, width: int, height: int, version: int = 2, header: bool = True) -> None:
    """A ``.dat`` file of ``records`` (uint32 [n, 2]): the ``%`` header with the version and the geometry, the event type and event
    size bytes, the records.  ``header=False``: the records alone, as headerless files are."""
    records = np.ascontiguousarray(np.asarray(records, dtype="<u4").reshape(-1, 2))
    with open(path, "wb") as f:
        if header:
            f.write(f"% Data file containing CD events.\n% Version {int(version)}\n% Height {int(height)}\n% Width {int(width)}\n"
                    .encode("ascii"))
            f.write(bytes([0x0C if version == 2 else 0x00, 8]))
        f.write(records.tobytes())


def read_header(path: str) -> RawHeader:
    """The header of a ``.raw`` or ``.dat`` file (``evt3.read_raw_header``).  A DAT file (the ``.dat`` suffix or ``% format DAT``) has
    format "DAT", its geometry from ``% Width`` / ``% Height``, and ``payload_offset`` past the event type and event size bytes that
    follow a header (a file without a header has neither; an event size other than 8 is refused)."""
    h = evt3.read_raw_header(path)
    if not (str(path).lower().endswith(".dat") or h.format == "DAT"):
        return h
    width, height = h.width, h.height
    if (width is None or height is None) and h.fields.get("Width", "").isdigit() and h.fields.get("Height", "").isdigit():
        width, height = int(h.fields["Width"]), int(h.fields["Height"])
    offset = h.payload_offset
    if offset > 0:
        with open(path, "rb") as f:
            f.seek(offset)
            two = f.read(2)
        if len(two) == 2:
            if two[1] != 8:
                raise ValueError(f"{path}: DAT event size {two[1]} is not decoded here, only 8-byte CD records")
            offset += 2
    return RawHeader("DAT", width, height, offset, h.fields)


def dat_version(header: RawHeader) -> int:
    """``% Version 1`` or ``2``; no version line: 2."""
    v = header.fields.get("Version", "2").strip()
    if v not in ("1", "2"):
        raise ValueError(f"DAT version {v!r} is not decoded here, only 1 and 2")
    return int(v)


def half_swapped_of(header: RawHeader, half_swapped: Optional[bool] = None) -> bool:
    """Whether an EVT 2.1 file holds the legacy order: the argument if given, else False for a format line with
    ``endianness=little`` and True otherwise."""
    if half_swapped is not None:
        return bool(half_swapped)
    options = [o.strip().lower() for o in header.fields.get("format", "").split(";")[1:]]
    return "endianness=little" not in options


# ---------------------------------------------------------------------------------------------------- decode (device)
def chunk_words(fmt: str = "EVT2") -> int:
    """Words per chunk of the decode (``ebos_evt2_chunk_words``): where the seams between workgroups lie."""
    return int(_hip.load_library().ebos_evt2_chunk_words(WORD_BYTES[fmt.upper()]))


def new_carry(device="cuda", state: Optional[dict] = None) -> torch.Tensor:
    """A decoder state on the device (``ebos_evt2_state`` as 16 bytes): the start state, or ``state``'s fields."""
    s = _hip.Evt2State(**(state or {}))
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(device)


def carry_to_dict(carry: torch.Tensor) -> dict:
    """The fields of a device decoder state (one read-back)."""
    s = _hip.Evt2State.from_buffer_copy(carry.cpu().numpy().tobytes())
    return {k: int(getattr(s, k)) for k, _ in _hip.Evt2State._fields_}


def _device_words(words, word_bytes: int, device) -> torch.Tensor:
    """Words of ``word_bytes`` bytes as a 1-D device tensor of the signed type of that size."""
    signed = torch.int32 if word_bytes == 4 else torch.int64
    if isinstance(words, torch.Tensor):
        if words.dim() != 1 or words.element_size() != word_bytes or words.is_floating_point():
            raise TypeError(f"words are a 1-D tensor of {word_bytes}-byte integers, got {words.dtype} {tuple(words.shape)}")
        return words.contiguous().view(signed).to(device)
    arr = np.ascontiguousarray(np.asarray(words))
    if arr.dtype != (np.uint32 if word_bytes == 4 else np.uint64) or arr.ndim != 1:
        raise TypeError(f"words are a 1-D uint{8 * word_bytes} array, got {arr.dtype} {arr.shape}")
    return torch.from_numpy(arr.view(np.int32 if word_bytes == 4 else np.int64)).to(device)


def evt2_scan(words: torch.Tensor, carry: Optional[torch.Tensor] = None, half_swapped: bool = False):
    """Passes 1 and 2 on a device tensor of words (int32: EVT 2.0, int64: EVT 2.1): (scratch, totals int64 [2] on the device, the
    carry-out).  No synchronisation."""
    lib = _hip.require_gpu()
    dev, n, wb = words.device, words.numel(), words.element_size()
    with _hip.on_device(dev):
        scratch = torch.empty(int(lib.ebos_evt2_scratch_bytes(n, wb)), dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        carry_out = torch.empty(C.sizeof(_hip.Evt2State), dtype=torch.uint8, device=dev)
        _hip.check(lib.ebos_evt2_scan(_hip.ptr(words) if n else None, n, wb, int(bool(half_swapped)), _hip.ptr(carry), _hip.ptr(carry_out),
                                      _hip.ptr(totals), _hip.ptr(scratch), scratch.numel(), _hip.stream_ptr(dev)), "ebos_evt2_scan")
    return scratch, totals, carry_out


def evt2_emit(words: torch.Tensor, scratch: torch.Tensor, n_events: int, n_triggers: int, x, y, t, p, trigger_t, trigger_value,
              trigger_id, half_swapped: bool = False) -> None:
    """Pass 3 into the caller's columns (their lengths are the capacities); ``scratch`` is what ``evt2_scan`` left for these words."""
    lib = _hip.require_gpu()
    n, wb = words.numel(), words.element_size()
    with _hip.on_device(words.device):
        _hip.check(lib.ebos_evt2_emit(_hip.ptr(words) if n else None, n, wb, int(bool(half_swapped)), _hip.ptr(scratch), scratch.numel(),
                                      int(n_events), int(n_triggers), min(c.numel() for c in (x, y, t, p)),
                                      min(c.numel() for c in (trigger_t, trigger_value, trigger_id)), _hip.ptr(x), _hip.ptr(y), _hip.ptr(t),
                                      _hip.ptr(p), _hip.ptr(trigger_t), _hip.ptr(trigger_value), _hip.ptr(trigger_id),
                                      _hip.stream_ptr(words.device)), "ebos_evt2_emit")


def set_evt21_route(route: int) -> int:
    """How the EVT 2.1 emit pass expands vector words (``ebos_evt21_route``: 0 the build's choice, 1 lane walk, 2 slot search); the
    previous value.  The output is the same either way."""
    before = int(_hip.load_library().ebos_evt21_route(int(route)))
    if before < 0:
        raise ValueError(f"route must be 0, 1 or 2, got {route}")
    return before


def _decode_words(words, word_bytes, carry, half_swapped, device) -> Evt2Slab:
    _hip.require_gpu()
    w = _device_words(words, word_bytes, device)
    scratch, totals, carry_out = evt2_scan(w, carry, half_swapped)
    n_ev, n_tr = (int(v) for v in totals.tolist())
    dev = w.device
    cols = [torch.empty(n_ev, dtype=d, device=dev) for d in (torch.int16, torch.int16, torch.int64, torch.uint8)]
    trig = [torch.empty(n_tr, dtype=d, device=dev) for d in (torch.int64, torch.uint8, torch.uint8)]
    evt2_emit(w, scratch, n_ev, n_tr, *cols, *trig, half_swapped=half_swapped)
    return Evt2Slab(*cols, *trig, carry_out)


def decode_evt2(words, carry: Optional[torch.Tensor] = None, device="cuda") -> Evt2Slab:
    """One slab of EVT 2.0 words (a host uint32 array or a device tensor) decoded from ``carry`` (None: the start state): the device
    columns x, y int16, t int64 (microseconds), p uint8, the triggers' t int64, value and id uint8, and the carry after the slab's
    last word, on the device.  One host read-back, of the two totals that size the columns."""
    return _decode_words(words, 4, carry, False, device)


def decode_evt21(words, carry: Optional[torch.Tensor] = None, half_swapped: bool = False, device="cuda") -> Evt2Slab:
    """The same for one slab of EVT 2.1 words (uint64); ``half_swapped``: the words hold the legacy order."""
    return _decode_words(words, 8, carry, half_swapped, device)


def decode_dat(records, version: int = 2, device="cuda"):
    """DAT records (a host uint32 array [n, 2] or flat [2 n], or a device int32 tensor of the same shapes) as the device columns x, y
    int16, t int64, p uint8."""
    lib = _hip.require_gpu()
    if isinstance(records, torch.Tensor):
        if records.element_size() != 4 or records.is_floating_point():
            raise TypeError(f"DAT records are 4-byte integers, got {records.dtype}")
        r = records.contiguous().view(torch.int32).reshape(-1).to(device)
    else:
        arr = np.ascontiguousarray(np.asarray(records))
        if arr.dtype != np.uint32:
            raise TypeError(f"DAT records are a uint32 array, got {arr.dtype}")
        r = torch.from_numpy(arr.reshape(-1).view(np.int32)).to(device)
    if r.numel() % 2:
        raise ValueError("DAT records are pairs of words (ts, data)")
    n = r.numel() // 2
    cols = [torch.empty(n, dtype=d, device=r.device) for d in (torch.int16, torch.int16, torch.int64, torch.uint8)]
    with _hip.on_device(r.device):
        _hip.check(lib.ebos_dat_decode(_hip.ptr(r) if n else None, n, int(version), *(_hip.ptr(c) for c in cols), n,
                                       _hip.stream_ptr(r.device)), "ebos_dat_decode")
    return tuple(cols)


def _payload_items(path: str, header: RawHeader, item_bytes: int, what: str) -> int:
    n_bytes = max(0, os.path.getsize(path) - header.payload_offset)
    if n_bytes % item_bytes:
        logger.warning(f"{path}: the payload ({n_bytes} bytes) is no whole number of {item_bytes}-byte {what}; "
                       f"the last {n_bytes % item_bytes} bytes are dropped")
    return n_bytes // item_bytes


def decode_recording(path: str, slab_words: int = 1 << 26, sensor_size: Optional[Tuple[int, int]] = None,
                     half_swapped: Optional[bool] = None, device="cuda"):
    """A ``.raw`` file of any format, or a ``.dat`` file, decoded slab by slab on the GPU: host columns (x int16, y int16, t int64,
    p uint8), the triggers as int64 [n, 3] = (t, id, value) (none in a DAT file), and the header (with ``sensor_size`` in the place
    of a missing geometry).  EVT 3.0 goes to ``evt3.decode_raw_file``; EVT 2.0 / 2.1 keep the carry on the device between slabs;
    ``half_swapped``: see ``half_swapped_of``.  A payload that is no whole number of words or records loses its tail with a warning."""
    header = read_header(path)
    if header.format == "EVT3":
        return evt3.decode_raw_file(path, slab_words=slab_words, sensor_size=sensor_size, device=device)
    if header.format not in ("EVT2", "EVT21", "DAT"):
        if header.format is None:
            raise ValueError(f"{path}: the header declares no format (`% evt 2.0`, `% evt 2.1`, `% evt 3.0` or a `% format` line)")
        raise NotImplementedError(f"{path}: format {header.format} is not decoded here, only EVT2, EVT21, EVT3 and DAT")
    if sensor_size is not None:
        header = header._replace(height=int(sensor_size[0]), width=int(sensor_size[1]))
    if header.width is None or header.height is None:
        raise ValueError(f"{path}: the header holds no geometry; pass sensor_size=(H, W)")
    if slab_words < 1 or slab_words > (1 << 30):
        raise ValueError(f"slab_words must lie in [1, 2^30], got {slab_words}")
    _hip.require_gpu()
    dtypes = (np.int16, np.int16, np.int64, np.uint8)
    cols, trigs = [[] for _ in range(4)], []
    with open(path, "rb") as f:
        f.seek(header.payload_offset)
        if header.format == "DAT":
            version = dat_version(header)
            n = _payload_items(path, header, 8, "records")
            for lo in range(0, n, int(slab_words)):
                records = np.fromfile(f, dtype="<u4", count=2 * min(int(slab_words), n - lo)).astype(np.uint32, copy=False)
                for k, c in enumerate(decode_dat(records, version, device)):
                    cols[k].append(c.cpu().numpy())
        else:
            wb = WORD_BYTES[header.format]
            swapped = half_swapped_of(header, half_swapped) if header.format == "EVT21" else False
            n = _payload_items(path, header, wb, "words")
            carry = None
            for lo in range(0, n, int(slab_words)):
                words = np.fromfile(f, dtype=f"<u{wb}", count=min(int(slab_words), n - lo)).astype(f"u{wb}", copy=False)
                slab = _decode_words(words, wb, carry, swapped, device)
                carry = slab.carry
                for k in range(4):
                    cols[k].append(slab[k].cpu().numpy())
                trigs.append(torch.stack([slab.trigger_t, slab.trigger_id.to(torch.int64), slab.trigger_value.to(torch.int64)], 1).cpu().numpy())
    x, y, t, p = (np.concatenate(c) if c else np.zeros(0, d) for c, d in zip(cols, dtypes))
    triggers = np.concatenate(trigs) if trigs else np.zeros((0, 3), np.int64)
    return x, y, t, p, triggers, header
