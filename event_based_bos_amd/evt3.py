"""Prophesee EVT 3.0 ``.raw`` recordings: the header and the encoder on the host, the decode on the GPU (csrc/evt3.hip).

The reference's recordings are ``prophesee_0/cd_events.raw`` (src/data_loader/ccs.py:171); its own ``.raw`` path through OpenEB's
``RawReader`` (:103-108, :299-317) is switched off in favour of a conversion to HDF5 (:19-20).  Here the file is read as it is:

    header = read_raw_header("cd_events.raw")                      # format, geometry, where the words begin
    x, y, t, p, triggers, header = decode_raw_file("cd_events.raw")   # host columns; triggers int64 [n, 3] = (t, id, value)
    slab = decode_evt3(words)                                      # one slab of uint16 words -> device columns + the carry

The word rules are those of include/ebos_hip.h.  There is no CPU decode: without a GPU ``decode_*`` raises ``HipUnavailableError``.
``encode_evt3`` / ``write_raw_file`` write streams (numpy, host) for tests, synthetic recordings and tools.  Neither OpenEB nor a
camera file was at hand: the decoder is checked against a restatement of the rules, not against OpenEB.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip, _word_stream as _ws
from ._word_stream import RawHeader, read_raw_header   # noqa: F401  (public here)

TIME_HIGH, TIME_LOW, ADDR_Y, ADDR_X, VECT_BASE_X, VECT_12, VECT_8, EXT_TRIGGER = 0x8, 0x6, 0x0, 0x2, 0x3, 0x4, 0x5, 0xA
_TH_STEP = 8   # the encoder's consecutive TIME_HIGH words differ by at most this many ticks of 4096 us

_FORMAT = _ws.WORDS["EVT3"]
Evt3Slab = _ws.Slab


# ---------------------------------------------------------------------------------------------------- files
_HINTS = ("`% evt 3.0` or `% format EVT3`", "EVT3 (EVT 3.0)", " (`% geometry WxH` or `% format EVT3;height=H;width=W`)")
_ODD_TAIL = "the payload has an odd length ({n_bytes} bytes); the last byte is dropped"


def _checked_header(path: str, sensor_size: Optional[Tuple[int, int]], slab_words: int = 1) -> RawHeader:
    return _ws.checked_header(path, read_raw_header(path), ("EVT3",), _HINTS, sensor_size, slab_words)


def raw_word_count(path: str, header: RawHeader) -> int:
    """The 16-bit words after the header; an odd trailing byte is dropped with a warning."""
    return _ws.payload_items(path, header, 2, "words", _ODD_TAIL)


def write_raw_file(path: str, words, width: int, height: int) -> None:
    """A ``.raw`` file of ``words`` (uint16) under the header current cameras write (``% format EVT3;height=H;width=W``, ``% end``)."""
    _ws.write_raw_file(path, words, width, height, "EVT3")


# ---------------------------------------------------------------------------------------------------- encoder (host)
def encode_evt3(x, y, t, p, triggers=None, vectorize: bool = True) -> np.ndarray:
    """The events (sensor x, y < 2048, t in microseconds and non-decreasing, polarity) and ``triggers`` (int [m, 3] = (t, id, value),
    t non-decreasing, id < 16) as EVT 3.0 words: a trigger goes after the events up to its time.  TIME_HIGH words are inserted so
    that consecutive ones never differ by more than 8 ticks -- starting from 0, so the decoder counts every wrap of the 24-bit time
    --; TIME_LOW and ADDR_Y come on change; runs of equal (t, y, p) with ascending x less than 12 apart are packed into VECT_BASE_X +
    VECT_12 words (a VECT_8 for a last group that fits) where ``vectorize`` allows, every other event is an ADDR_X."""
    x, y, t, p = _ws.columns(x, y, t, p)
    trig = _ws.trigger_rows(triggers, 4, "EVT3")
    n = len(t)
    if n and (x.min() < 0 or x.max() > 0x7FF or y.min() < 0 or y.max() > 0x7FF):
        raise ValueError("EVT3 addresses are 11 bits: 0 <= x, y < 2048")
    is_trig, it = _ws.merge(t, trig)
    total = n + len(trig)
    if total == 0:
        return np.zeros(0, np.uint16)
    ev_pos = np.nonzero(~is_trig)[0]
    # TIME_HIGH ramps: from the previous item's high part (0 before the first item, which always gets at least one word)
    high = it >> 12
    gap = np.diff(np.concatenate(([0], high)))
    n_th = (gap + _TH_STEP - 1) // _TH_STEP
    n_th[0] = max(int(n_th[0]), 1)
    low = it & 0xFFF
    prev_low = np.concatenate(([0], low[:-1]))
    c_tl = np.where(n_th > 0, low != 0, low != prev_low)
    # ADDR_Y: an event whose row differs from the event before it
    c_y = np.zeros(total, bool)
    if n:
        c_y[ev_pos] = np.concatenate(([True], y[1:] != y[:-1]))
    # vector runs: an event continues the run of the event right before it (no trigger between)
    c_main = np.ones(total, bool)      # ADDR_X, EXT_TRIGGER or VECT_BASE_X
    c_vec = np.zeros(total, bool)      # a vector word, placed at the first event of its group of 12
    main = np.zeros(total, np.int64)
    vec = np.zeros(total, np.int64)
    main[is_trig] = (EXT_TRIGGER << 12) | (trig[:, 1] << 8) | (trig[:, 2] & 1)
    main[ev_pos] = (ADDR_X << 12) | (p << 11) | x
    if n and vectorize:
        cont = np.zeros(n, bool)
        cont[1:] = ((t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & (x[1:] > x[:-1]) & (x[1:] - x[:-1] < 12) &
                    (ev_pos[1:] == ev_pos[:-1] + 1))
        run = np.cumsum(~cont) - 1
        run_start = np.nonzero(~cont)[0]
        run_len = np.diff(np.concatenate((run_start, [n])))
        in_vec = run_len[run] >= 2
        rel = x - x[run_start][run]
        group = rel // 12
        first_of_group = in_vec & np.concatenate(([True], (run[1:] != run[:-1]) | (group[1:] != group[:-1])))
        gid = np.cumsum(first_of_group) - 1
        mask = np.zeros(int(first_of_group.sum()), np.int64)
        np.add.at(mask, gid[in_vec], np.int64(1) << (rel[in_vec] % 12))
        gstart = np.nonzero(first_of_group)[0]
        last_group = np.concatenate((run[gstart][1:] != run[gstart][:-1], [True])) if len(gstart) else np.zeros(0, bool)
        kind = np.where(last_group & (mask < 256), VECT_8, VECT_12)
        starts_run = in_vec & ~cont
        c_main[ev_pos[in_vec & cont]] = False
        main[ev_pos[starts_run]] = (VECT_BASE_X << 12) | (p[starts_run] << 11) | x[starts_run]
        c_vec[ev_pos[gstart]] = True
        vec[ev_pos[gstart]] = (kind << 12) | mask
    counts = n_th + c_tl + c_y + c_main + c_vec
    offs = np.concatenate(([0], np.cumsum(counts)))
    out = np.zeros(int(offs[-1]), np.int64)
    # the ramps: word k (1-based) of item i's ramp is min(prev_high + 8 k, high_i)
    th_total = int(n_th.sum())
    owner = np.repeat(np.arange(total), n_th)
    k = np.arange(th_total) - np.repeat(np.cumsum(n_th) - n_th, n_th) + 1
    prev_high = np.concatenate(([0], high[:-1]))
    out[offs[owner] + k - 1] = (TIME_HIGH << 12) | (np.minimum(prev_high[owner] + _TH_STEP * k, high[owner]) & 0xFFF)
    at = offs[:-1] + n_th
    out[at[c_tl]] = (TIME_LOW << 12) | low[c_tl]
    at = at + c_tl
    if n:
        rows = np.zeros(total, np.int64)
        rows[ev_pos] = y
        out[at[c_y]] = (ADDR_Y << 12) | rows[c_y]
    at = at + c_y
    out[at[c_main]] = main[c_main]
    at = at + c_main
    out[at[c_vec]] = vec[c_vec]
    return out.astype(np.uint16)


# ---------------------------------------------------------------------------------------------------- decode (device)
def chunk_words() -> int:
    """Words per chunk of the decode (``ebos_evt3_chunk_words``): where the seams between workgroups lie."""
    return _ws.chunk_words(_FORMAT)


def new_carry(device="cuda", state: Optional[dict] = None) -> torch.Tensor:
    """A decoder state on the device (``ebos_evt3_state`` as 32 bytes): the start state, or ``state``'s fields."""
    return _ws.new_carry(_FORMAT, device, state)


def carry_to_dict(carry: torch.Tensor) -> dict:
    """The fields of a device decoder state (one read-back)."""
    return _ws.carry_to_dict(_FORMAT, carry)


def _device_words(words, device) -> torch.Tensor:
    if isinstance(words, torch.Tensor):
        if words.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or words.dim() != 1:
            raise TypeError(f"EVT3 words are a 1-D uint16 (or int16) tensor, got {words.dtype} {tuple(words.shape)}")
        return words.contiguous().to(device)
    arr = np.ascontiguousarray(np.asarray(words))
    if arr.dtype != np.uint16 or arr.ndim != 1:
        raise TypeError(f"EVT3 words are a 1-D uint16 array, got {arr.dtype} {arr.shape}")
    return torch.from_numpy(arr.view(_FORMAT.np_signed)).to(device)


def evt3_scan(words: torch.Tensor, carry: Optional[torch.Tensor] = None):
    """Passes 1 and 2 on a device tensor of words: (scratch, totals int64 [2] on the device, the carry-out).  No synchronisation."""
    return _ws.scan(_FORMAT, words, carry)


def evt3_emit(words: torch.Tensor, scratch: torch.Tensor, n_events: int, n_triggers: int, x, y, t, p, trigger_t, trigger_value,
              trigger_id) -> None:
    """Pass 3 into the caller's columns (their lengths are the capacities); ``scratch`` is what ``evt3_scan`` left for these words."""
    _ws.emit(_FORMAT, words, scratch, n_events, n_triggers, x, y, t, p, trigger_t, trigger_value, trigger_id)


def decode_evt3(words, carry: Optional[torch.Tensor] = None, device="cuda") -> Evt3Slab:
    """One slab of EVT 3.0 words (a host uint16 array or a device tensor) decoded from ``carry`` (None: the start state): the device
    columns x, y int16, t int64 (microseconds), p uint8, the triggers' t int64, value and id uint8, and the carry after the slab's
    last word, on the device.  One host read-back, of the two totals that size the columns."""
    _hip.require_gpu()
    return _ws.decode_slab(_FORMAT, _device_words(words, device), carry)


def decode_raw_file(path: str, slab_words: int = 1 << 26, sensor_size: Optional[Tuple[int, int]] = None, device="cuda"):
    """A ``.raw`` file decoded slab by slab, the carry staying on the device between slabs: host columns (x int16, y int16, t int64,
    p uint8), the triggers as int64 [n, 3] = (t, id, value), and the header (with ``sensor_size`` in the place of a missing
    geometry).  An odd trailing byte is dropped with a warning."""
    header = _checked_header(path, sensor_size, slab_words)
    return _ws.decode_file(path, header, slab_words, lambda words, carry: decode_evt3(words, carry, device), 2, tail=_ODD_TAIL)
