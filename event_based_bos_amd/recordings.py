"""Prophesee recordings in every format the cameras and tools write: EVT 2.0, EVT 2.1 and EVT 3.0 ``.raw`` files and ``.dat``
files.  The headers and the encoders are host code (numpy); the decode runs on the GPU (csrc/evt2.hip; EVT 3.0: csrc/evt3.hip,
``evt3.py``), every format through the one slab decode and the one file loop of ``_word_stream.py``.

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

from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip, _word_stream as _ws, evt3
from ._word_stream import RawHeader
from ._word_stream import payload_items as _payload_items   # noqa: F401  (tests/test_recordings.py reads the warning through it)

TIME_HIGH, CD_OFF, CD_ON, EXT_TRIGGER = 0x8, 0x0, 0x1, 0xA
_TH_MASK = (1 << 28) - 1
WORD_BYTES = {"EVT2": 4, "EVT21": 8}
FORMATS = ("EVT2", "EVT21", "EVT3", "DAT")
_HINTS = ("`% evt 2.0`, `% evt 2.1`, `% evt 3.0` or a `% format` line", "EVT2, EVT21, EVT3 and DAT", "")

Evt2Slab = _ws.Slab


# ---------------------------------------------------------------------------------------------------- encoders (host)
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
    x, y, t, p = _ws.columns(x, y, t, p)
    trig = _ws.trigger_rows(triggers, 5, "EVT2")
    if len(t) and (x.min() < 0 or x.max() > 0x7FF or y.min() < 0 or y.max() > 0x7FF):
        raise ValueError("EVT2 addresses are 11 bits: 0 <= x, y < 2048")
    is_trig, it = _ws.merge(t, trig)
    main = np.zeros(len(it), np.int64)
    main[is_trig] = (EXT_TRIGGER << 28) | (trig[:, 1] << 8) | (trig[:, 2] & 1)
    main[~is_trig] = (p << 28) | (x << 11) | y
    main |= (it & 0x3F) << 22
    return _with_time_high(it, main.astype(np.uint64), 0).astype(np.uint32)


def encode_evt21(x, y, t, p, triggers=None, vectorize: bool = True) -> np.ndarray:
    """The same as EVT 2.1 words (uint64, plain order).  ``vectorize``: a run of consecutive events of equal (t, y, p) whose x
    ascend inside one 32-aligned block becomes one word of base ``x & ~31``; otherwise every event is a word of base x, mask 1."""
    x, y, t, p = _ws.columns(x, y, t, p)
    trig = _ws.trigger_rows(triggers, 5, "EVT2")
    n = len(t)
    if n and (x.min() < 0 or x.max() > 0x7FF or y.min() < 0 or y.max() > 0x7FF):
        raise ValueError("EVT2.1 addresses are 11 bits: 0 <= x, y < 2048")
    is_trig, it = _ws.merge(t, trig)
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
    x, y, t, p = _ws.columns(x, y, t, p)
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
    if fmt != "EVT3" and fmt not in WORD_BYTES:
        raise ValueError(f"write_raw_file writes EVT2, EVT21 and EVT3, not {fmt}")
    _ws.write_raw_file(path, words, width, height, fmt)


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
    h = _ws.read_raw_header(path)
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
_BY_SIZE = {f.word_bytes: f for f in map(_ws.WORDS.get, WORD_BYTES)}


def chunk_words(fmt: str = "EVT2") -> int:
    """Words per chunk of the decode (``ebos_evt2_chunk_words``): where the seams between workgroups lie."""
    return _ws.chunk_words(_BY_SIZE[WORD_BYTES[fmt.upper()]])


def new_carry(device="cuda", state: Optional[dict] = None) -> torch.Tensor:
    """A decoder state on the device (``ebos_evt2_state`` as 16 bytes): the start state, or ``state``'s fields."""
    return _ws.new_carry(_BY_SIZE[4], device, state)


def carry_to_dict(carry: torch.Tensor) -> dict:
    """The fields of a device decoder state (one read-back)."""
    return _ws.carry_to_dict(_BY_SIZE[4], carry)


def _device_words(words, word_bytes: int, device) -> torch.Tensor:
    """Words of ``word_bytes`` bytes as a 1-D device tensor of the signed type of that size."""
    f = _BY_SIZE[word_bytes]
    if isinstance(words, torch.Tensor):
        if words.dim() != 1 or words.element_size() != word_bytes or words.is_floating_point():
            raise TypeError(f"words are a 1-D tensor of {word_bytes}-byte integers, got {words.dtype} {tuple(words.shape)}")
        return words.contiguous().view(f.torch_signed).to(device)
    arr = np.ascontiguousarray(np.asarray(words))
    if arr.dtype != np.dtype(f"u{word_bytes}") or arr.ndim != 1:
        raise TypeError(f"words are a 1-D uint{8 * word_bytes} array, got {arr.dtype} {arr.shape}")
    return torch.from_numpy(arr.view(f.np_signed)).to(device)


def evt2_scan(words: torch.Tensor, carry: Optional[torch.Tensor] = None, half_swapped: bool = False):
    """Passes 1 and 2 on a device tensor of words (int32: EVT 2.0, int64: EVT 2.1): (scratch, totals int64 [2] on the device, the
    carry-out).  No synchronisation."""
    return _ws.scan(_BY_SIZE[words.element_size()], words, carry, half_swapped)


def evt2_emit(words: torch.Tensor, scratch: torch.Tensor, n_events: int, n_triggers: int, x, y, t, p, trigger_t, trigger_value,
              trigger_id, half_swapped: bool = False) -> None:
    """Pass 3 into the caller's columns (their lengths are the capacities); ``scratch`` is what ``evt2_scan`` left for these words."""
    _ws.emit(_BY_SIZE[words.element_size()], words, scratch, n_events, n_triggers, x, y, t, p, trigger_t, trigger_value, trigger_id, half_swapped)


def _decode_words(words, word_bytes, carry, half_swapped, device) -> Evt2Slab:
    _hip.require_gpu()
    return _ws.decode_slab(_BY_SIZE[word_bytes], _device_words(words, word_bytes, device), carry, half_swapped)


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
    cols = [torch.empty(n, dtype=d, device=r.device) for d in _ws.COLUMNS]
    with _hip.on_device(r.device):
        _hip.check(lib.ebos_dat_decode(_hip.ptr(r) if n else None, n, int(version), *(_hip.ptr(c) for c in cols), n,
                                       _hip.stream_ptr(r.device)), "ebos_dat_decode")
    return tuple(cols)


def decode_recording(path: str, slab_words: int = 1 << 26, sensor_size: Optional[Tuple[int, int]] = None,
                     half_swapped: Optional[bool] = None, device="cuda"):
    """A ``.raw`` file of any format, or a ``.dat`` file, decoded slab by slab on the GPU: host columns (x int16, y int16, t int64,
    p uint8), the triggers as int64 [n, 3] = (t, id, value) (none in a DAT file), and the header (with ``sensor_size`` in the place
    of a missing geometry).  EVT 3.0 goes to ``evt3.decode_raw_file``; EVT 2.0 / 2.1 keep the carry on the device between slabs;
    ``half_swapped``: see ``half_swapped_of``.  A payload that is no whole number of words or records loses its tail with a warning."""
    header = read_header(path)
    if header.format == "EVT3":
        return evt3.decode_raw_file(path, slab_words=slab_words, sensor_size=sensor_size, device=device)
    header = _ws.checked_header(path, header, FORMATS, _HINTS, sensor_size, slab_words)
    if header.format == "DAT":      # a slab of records: no carry, no triggers
        version = dat_version(header)

        def decode(records, carry):
            return Evt2Slab(*decode_dat(records, version, device), *(torch.empty(0, dtype=d, device=device) for d in _ws.TRIGGERS), None)
        return _ws.decode_file(path, header, slab_words, decode, 4, 2, "records")
    wb = WORD_BYTES[header.format]
    swapped = half_swapped_of(header, half_swapped) if header.format == "EVT21" else False
    return _ws.decode_file(path, header, slab_words, lambda w, carry: _decode_words(w, wb, carry, swapped, device), wb)
