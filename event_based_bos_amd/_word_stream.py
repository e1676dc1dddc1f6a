"""What the readers of Prophesee recordings share (``evt3.py``: EVT 3.0; ``recordings.py``: EVT 2.0, EVT 2.1 and DAT): the header of a
``.raw`` file, the first steps of the encoders, one table of the word formats, one slab decode on the GPU driven by that table
(csrc/evt3.hip, csrc/evt2.hip) and one loop over the slabs of a file.  Private: the public names are those of the two modules.
"""
from __future__ import annotations

import ctypes as C
import functools
import logging
import os
import re
from collections import namedtuple
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _hip

logger = logging.getLogger(__name__)

RawHeader = namedtuple("RawHeader", "format width height payload_offset fields")
Slab = namedtuple("Slab", "x y t p trigger_t trigger_value trigger_id carry")

# a word format: the word's size and signed types, the ctypes mirror of its decoder state, its C entries by name and the integer
# arguments they take after n_words (ebos_evt2_*: the word size; their scan and emit also whether the halves are exchanged: `extra`
# is indexed by that flag)
Format = namedtuple("Format", "word_bytes np_signed torch_signed state state_bytes chunk_words scratch_bytes scan emit size_args extra")


def _format(word_bytes, np_signed, torch_signed, state, prefix, size_args):
    extra = tuple(size_args + (k,) for k in (0, 1)) if size_args else ((), ())
    return Format(word_bytes, np_signed, torch_signed, state, C.sizeof(state), *(f"{prefix}_{e}" for e in ("chunk_words", "scratch_bytes", "scan", "emit")),
                  size_args, extra)


WORDS = {"EVT2": _format(4, np.int32, torch.int32, _hip.Evt2State, "ebos_evt2", (4,)),
         "EVT21": _format(8, np.int64, torch.int64, _hip.Evt2State, "ebos_evt2", (8,)),
         "EVT3": _format(2, np.int16, torch.int16, _hip.Evt3State, "ebos_evt3", ())}

COLUMNS = (torch.int16, torch.int16, torch.int64, torch.uint8)
TRIGGERS = (torch.int64, torch.uint8, torch.uint8)


# ---------------------------------------------------------------------------------------------------- encoders' first steps (host)
def columns(x, y, t, p):
    """x, y, t and the polarity as 0 / 1, flat int64 columns of one length; t non-negative and non-decreasing."""
    x, y, p = (np.asarray(a).astype(np.int64).ravel() for a in (x, y, p))
    t = np.asarray(t).astype(np.int64).ravel()
    if not (len(x) == len(y) == len(p) == len(t)):
        raise ValueError("x, y, t, p must be of equal length")
    if len(t) and (t[0] < 0 or np.any(np.diff(t) < 0)):
        raise ValueError("t must be non-negative and non-decreasing")
    return x, y, t, (p != 0).astype(np.int64)


def trigger_rows(triggers, id_bits: int, name: str):
    """``triggers`` as int64 [m, 3] = (t, id, value), the ids within ``name``'s ``id_bits`` bits."""
    trig = np.zeros((0, 3), np.int64) if triggers is None else np.asarray(triggers, dtype=np.int64).reshape(-1, 3)
    if len(trig) and (trig[:, 1].min() < 0 or trig[:, 1].max() >> id_bits):
        raise ValueError(f"{name} trigger ids are {id_bits} bits")
    if len(trig) and (trig[0, 0] < 0 or np.any(np.diff(trig[:, 0]) < 0)):
        raise ValueError("trigger t must be non-negative and non-decreasing")
    return trig


def merge(t, trig):
    """The merged items: trigger j sits after the events with t <= its time.  (is_trig [total], item time [total])"""
    n, m = len(t), len(trig)
    trig_pos = np.searchsorted(t, trig[:, 0], side="right") + np.arange(m)
    is_trig = np.zeros(n + m, bool)
    is_trig[trig_pos] = True
    it = np.empty(n + m, np.int64)
    it[is_trig], it[~is_trig] = trig[:, 0], t
    return is_trig, it


# ---------------------------------------------------------------------------------------------------- headers
def write_raw_file(path: str, words, width: int, height: int, fmt: str) -> None:
    """A ``.raw`` file of ``words`` under the header current cameras write for ``fmt`` (EVT 2.1: the plain order, declared)."""
    version, option = {"EVT2": ("2.0", ""), "EVT21": ("2.1", "endianness=little;"), "EVT3": ("3.0", "")}[fmt]
    words = np.ascontiguousarray(np.asarray(words, dtype=f"<u{WORDS[fmt].word_bytes}"))
    with open(path, "wb") as f:
        f.write(f"% camera_integrator_name Prophesee\n% evt {version}\n% format {fmt};{option}height={int(height)};width={int(width)}\n"
                f"% geometry {int(width)}x{int(height)}\n% end\n".encode("ascii"))
        f.write(words.tobytes())


def read_raw_header(path: str) -> RawHeader:
    """The ASCII header of a ``.raw`` file: while the next byte is ``%``, a line through the next newline; ``% end`` ends the header
    even if more ``%`` lines follow.  ``format`` is "EVT3" (``% evt 3.0`` or ``% format EVT3[;height=H;width=W]``) or the name of
    the format the file declares (None: none declared); the geometry comes from the format line's ``height=`` / ``width=`` or from
    ``% geometry WxH`` (None: none declared).  ``fields``: the raw ``key -> value`` strings."""
    fields: Dict[str, str] = {}
    with open(path, "rb") as f:
        offset = 0
        while True:
            c = f.read(1)
            if c != b"%":
                break
            line = c + f.readline()
            offset += len(line)
            f.seek(offset)
            text = line[1:].decode("ascii", "replace").strip()
            if text == "end":
                break
            key, _, value = text.partition(" ")
            if key:
                fields[key] = value.strip()
    fmt, width, height = None, None, None
    if "evt" in fields:
        fmt = {"3.0": "EVT3", "2.0": "EVT2", "2.1": "EVT21"}.get(fields["evt"], "evt " + fields["evt"])
    if "format" in fields:
        parts = fields["format"].split(";")
        fmt = parts[0].strip().upper()
        for part in parts[1:]:
            k, _, v = part.partition("=")
            if k.strip() == "height" and v.strip().isdigit():
                height = int(v)
            elif k.strip() == "width" and v.strip().isdigit():
                width = int(v)
    if (width is None or height is None) and "geometry" in fields:
        m = re.fullmatch(r"(\d+)\s*[xX]\s*(\d+)", fields["geometry"])
        if m:
            width, height = int(m.group(1)), int(m.group(2))
    return RawHeader(fmt, width, height, offset, fields)


def checked_header(path: str, header: RawHeader, accepted, hints, sensor_size: Optional[Tuple[int, int]], slab_words: int) -> RawHeader:
    """``header`` if the file can be decoded -- a declared format among ``accepted``, a geometry (``sensor_size`` = (H, W) in its
    place if given), ``slab_words`` in range -- or the refusal, worded by the caller's ``hints`` = (how a format is declared, the
    formats decoded, how a geometry is declared)."""
    declare, decoded, geometry = hints
    if header.format not in accepted:
        if header.format is None:
            raise ValueError(f"{path}: the header declares no format ({declare})")
        raise NotImplementedError(f"{path}: format {header.format} is not decoded here, only {decoded}")
    if sensor_size is not None:
        header = header._replace(height=int(sensor_size[0]), width=int(sensor_size[1]))
    if header.width is None or header.height is None:
        raise ValueError(f"{path}: the header holds no geometry{geometry}; pass sensor_size=(H, W)")
    if slab_words < 1 or slab_words > (1 << 30):
        raise ValueError(f"slab_words must lie in [1, 2^30], got {slab_words}")
    return header


def payload_items(path: str, header: RawHeader, item_bytes: int, what: str, tail: Optional[str] = None) -> int:
    """The whole items of ``item_bytes`` bytes after the header; a tail that is no whole item is dropped with a warning (``tail``:
    the caller's wording of it, with ``{n_bytes}``)."""
    n_bytes = max(0, os.path.getsize(path) - header.payload_offset)
    if n_bytes % item_bytes:
        tail = tail or f"the payload ({{n_bytes}} bytes) is no whole number of {item_bytes}-byte {what}; the last {n_bytes % item_bytes} bytes are dropped"
        logger.warning(f"{path}: " + tail.format(n_bytes=n_bytes))
    return n_bytes // item_bytes


# ---------------------------------------------------------------------------------------------------- one slab (device)
def chunk_words(f: Format) -> int:
    return int(getattr(_hip.load_library(), f.chunk_words)(*f.size_args))


@functools.lru_cache(maxsize=256)
def _scratch_bytes(f: Format, n: int) -> int:
    """(remembered: the slabs of a file are of one length, and the answer costs a call into the library)"""
    return int(getattr(_hip.load_library(), f.scratch_bytes)(n, *f.size_args))


def new_carry(f: Format, device="cuda", state: Optional[dict] = None) -> torch.Tensor:
    s = f.state(**(state or {}))
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(device)


def carry_to_dict(f: Format, carry: torch.Tensor) -> dict:
    s = f.state.from_buffer_copy(carry.cpu().numpy().tobytes())
    return {k: int(getattr(s, k)) for k, _ in f.state._fields_}


def scan(f: Format, words: torch.Tensor, carry: Optional[torch.Tensor] = None, half_swapped: bool = False):
    lib = _hip.require_gpu()
    dev, n = words.device, words.numel()
    with _hip.on_device(dev):
        scratch = torch.empty(_scratch_bytes(f, n), dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        carry_out = torch.empty(f.state_bytes, dtype=torch.uint8, device=dev)
        _hip.check(getattr(lib, f.scan)(_hip.ptr(words) if n else None, n, *f.extra[bool(half_swapped)], _hip.ptr(carry), _hip.ptr(carry_out),
                                         _hip.ptr(totals), _hip.ptr(scratch), scratch.numel(), _hip.stream_ptr(dev)), f.scan)
    return scratch, totals, carry_out


def emit(f: Format, words: torch.Tensor, scratch: torch.Tensor, n_events: int, n_triggers: int, x, y, t, p, trigger_t, trigger_value,
         trigger_id, half_swapped: bool = False) -> None:
    lib = _hip.require_gpu()
    n = words.numel()
    with _hip.on_device(words.device):
        _hip.check(getattr(lib, f.emit)(_hip.ptr(words) if n else None, n, *f.extra[bool(half_swapped)], _hip.ptr(scratch), scratch.numel(),
                                        int(n_events), int(n_triggers), min(x.numel(), y.numel(), t.numel(), p.numel()),
                                        min(trigger_t.numel(), trigger_value.numel(), trigger_id.numel()), _hip.ptr(x), _hip.ptr(y), _hip.ptr(t),
                                        _hip.ptr(p), _hip.ptr(trigger_t), _hip.ptr(trigger_value), _hip.ptr(trigger_id),
                                        _hip.stream_ptr(words.device)), f.emit)


def decode_slab(f: Format, w: torch.Tensor, carry: Optional[torch.Tensor] = None, half_swapped: bool = False) -> Slab:
    """One slab of words (a device tensor) decoded from ``carry`` (None: the start state).  One host read-back, of the two totals
    that size the columns."""
    scratch, totals, carry_out = scan(f, w, carry, half_swapped)
    n_ev, n_tr = (int(v) for v in totals.tolist())
    cols = [torch.empty(n_ev, dtype=d, device=w.device) for d in COLUMNS]
    trig = [torch.empty(n_tr, dtype=d, device=w.device) for d in TRIGGERS]
    emit(f, w, scratch, n_ev, n_tr, *cols, *trig, half_swapped=half_swapped)
    return Slab(*cols, *trig, carry_out)


# ---------------------------------------------------------------------------------------------------- one file
def decode_file(path: str, header: RawHeader, slab_words: int, decode, unit: int, per_item: int = 1, what: str = "words",
                tail: Optional[str] = None):
    """The payload after a checked ``header`` decoded slab by slab, ``slab = decode(items, carry)`` on ``slab_words`` items of
    ``per_item`` little-endian unsigned integers of ``unit`` bytes, the carry staying on the device between slabs: host columns (x
    int16, y int16, t int64, p uint8), the triggers as int64 [n, 3] = (t, id, value), and the header."""
    _hip.require_gpu()
    n = payload_items(path, header, unit * per_item, what, tail)
    carry = None
    cols, trigs = [[] for _ in range(4)], []
    with open(path, "rb") as fh:
        fh.seek(header.payload_offset)
        for lo in range(0, n, int(slab_words)):
            items = np.fromfile(fh, dtype=f"<u{unit}", count=per_item * min(int(slab_words), n - lo)).astype(f"u{unit}", copy=False)
            slab = decode(items, carry)
            carry = slab.carry
            for k in range(4):
                cols[k].append(slab[k].cpu().numpy())
            trigs.append(torch.stack([slab.trigger_t, slab.trigger_id.to(torch.int64), slab.trigger_value.to(torch.int64)], 1).cpu().numpy())
    dtypes = (np.int16, np.int16, np.int64, np.uint8)
    x, y, t, p = (np.concatenate(c) if c else np.zeros(0, d) for c, d in zip(cols, dtypes))
    triggers = np.concatenate(trigs) if trigs else np.zeros((0, 3), np.int64)
    return x, y, t, p, triggers, header
