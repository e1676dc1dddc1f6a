"""EVT 2.0, EVT 2.1 and DAT recordings, the host side: the sequential restatement of the word rules (tests/_evt2_ref.py) on the
worked examples, the package's encoders read back through it, the headers, the C entries' refusals and the state algebra of
csrc/evt2_core.h compiled for the host -- nothing here needs a GPU."""
import ctypes
import logging
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import _evt2_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


def rows(items):
    return [list(v) for v in items]


def test_worked_examples_through_the_restatement():
    e, t, s = ref.decode_evt2(ref.EVT2_EXAMPLE_WORDS)
    assert e.tolist() == rows(ref.EVT2_EXAMPLE_EVENTS) and t.tolist() == rows(ref.EVT2_EXAMPLE_TRIGGERS)
    assert s == dict(has_th=1, th=2, loops=0)
    e, t, s = ref.decode_evt21(ref.EVT21_EXAMPLE_WORDS)
    assert e.tolist() == rows(ref.EVT21_EXAMPLE_EVENTS) and t.tolist() == rows(ref.EVT21_EXAMPLE_TRIGGERS)
    assert s == dict(has_th=1, th=2, loops=0)
    swapped = [((w << 32) | (w >> 32)) & 0xFFFFFFFFFFFFFFFF for w in ref.EVT21_EXAMPLE_WORDS]
    assert ref.decode_evt21(swapped, half_swapped=True)[0].tolist() == rows(ref.EVT21_EXAMPLE_EVENTS)
    assert ref.decode_dat(ref.DAT2_EXAMPLE_RECORDS, 2).tolist() == rows(ref.DAT2_EXAMPLE_EVENTS)
    assert ref.decode_dat(ref.DAT1_EXAMPLE_RECORDS, 1).tolist() == rows(ref.DAT1_EXAMPLE_EVENTS)
    # a wrap needs a fall of at least 2^28 - 11; a smaller step backwards is kept as it is
    ev = 0x10000000
    assert ref.decode_evt2([0x8FFFFFFF, 0x80000000, ev])[0].tolist() == [[0, 0, 1 << 34, 1]]
    assert ref.decode_evt2([0x8FFFFFF5, 0x80000000, ev])[0].tolist() == [[0, 0, 1 << 34, 1]]
    assert ref.decode_evt2([0x8FFFFFF4, 0x80000000, ev])[0].tolist() == [[0, 0, 0, 1]]


def recording(seed, n=3000, t0=0):
    """Columns with duplicates, bursts of equal time, runs of ascending x on one row and wraps of the 34-bit time."""
    rng = np.random.default_rng(seed)
    t = t0 + np.cumsum(rng.choice([0, 0, 0, 1, 3, 700, 5000], size=n))
    t[n // 3:] += 2 * (1 << 34)                     # two wraps at once
    y = np.repeat(rng.integers(0, 720, size=n // 6 + 1), 6)[:n]
    x = rng.integers(0, 1280, size=n)
    for i in range(0, n - 8, 8):
        lo = int(x[i]) % 1200
        x[i:i + 6] = np.sort(rng.choice(np.arange(lo, lo + 40), 6, replace=False))
    x[5::50] = x[4::50][:len(x[5::50])]             # duplicates: the same pixel twice in a row
    y[5::50] = y[4::50][:len(y[5::50])]
    p = np.repeat(rng.integers(0, 2, size=n // 3 + 1), 3)[:n]
    m = 23
    triggers = np.stack([np.sort(rng.integers(int(t[0]), int(t[-1]) + 100, size=m)), rng.integers(0, 32, size=m),
                         rng.integers(0, 2, size=m)], 1)
    return x, y, t, p, triggers


T0 = [0, (1 << 34) - 3000]


@pytest.mark.parametrize("t0", T0, ids=["from0", "below2^34"])
def test_evt2_encoder_round_trip_through_the_restatement(t0):
    from event_based_bos_amd import recordings

    x, y, t, p, triggers = recording(3, t0=t0)
    assert t0 == 0 or (t[0] < (1 << 34) <= t[len(t) // 3 - 1])       # a wrap lies inside, apart from the two at the jump
    words = recordings.encode_evt2(x, y, t, p, triggers)
    assert words.dtype == np.uint32 and words[0] >> 28 == ref.TIME_HIGH
    events, trig, state = ref.decode_evt2(words)
    assert np.array_equal(events, np.stack([x, y, t, p], 1)) and np.array_equal(trig[:, [0, 2, 1]], triggers)
    assert state["loops"] == max(t[-1], triggers[-1, 0]) >> 34 >= 2
    # a wrap is the pair TIME_HIGH(2^28 - 1), TIME_HIGH(0): no ramp of words
    assert len(words) < 2 * (len(t) + len(triggers)) + 20


@pytest.mark.parametrize("t0", T0, ids=["from0", "below2^34"])
@pytest.mark.parametrize("vectorize", [True, False])
def test_evt21_encoder_round_trip_through_the_restatement(t0, vectorize):
    from event_based_bos_amd import recordings

    x, y, t, p, triggers = recording(4, t0=t0)
    words = recordings.encode_evt21(x, y, t, p, triggers, vectorize=vectorize)
    assert words.dtype == np.uint64
    is_event = (words >> np.uint64(60)) <= 1
    bits = np.array([bin(int(v)).count("1") for v in words[is_event] & np.uint64(0xFFFFFFFF)])
    assert int(bits.sum()) == len(t) and (bits.max() > 1) == vectorize
    if vectorize:
        assert np.all(((words[is_event] >> np.uint64(43)) & np.uint64(31)) == 0)      # 32-aligned bases
    events, trig, state = ref.decode_evt21(words)
    assert np.array_equal(events, np.stack([x, y, t, p], 1)) and np.array_equal(trig[:, [0, 2, 1]], triggers)
    assert state["loops"] >= 2


@pytest.mark.parametrize("version", [1, 2])
def test_dat_encoder_round_trip_through_the_restatement(version):
    from event_based_bos_amd import recordings

    x, y, t, p, _ = recording(5)
    t = t - t[len(t) // 3] + (1 << 31)              # inside 32 bits, past 2^31
    t[:len(t) // 3] = np.sort(t[:len(t) // 3] % 1000)
    if version == 1:
        x, y = x % 512, y % 256
    else:
        x[:3], y[:3] = [16383, 0, 16383], [0, 16383, 16383]
    records = recordings.encode_dat(x, y, t, p, version)
    assert records.dtype == np.uint32 and records.shape == (len(t), 2)
    assert np.array_equal(ref.decode_dat(records, version), np.stack([x, y, t, p], 1))


def test_encoders_refuse_what_the_formats_cannot_hold():
    from event_based_bos_amd import recordings as r

    assert len(r.encode_evt2([], [], [], [])) == 0 and len(r.encode_evt21([], [], [], [])) == 0 and r.encode_dat([], [], [], []).shape == (0, 2)
    for enc in (r.encode_evt2, r.encode_evt21):
        with pytest.raises(ValueError, match="11 bits"):
            enc([2048], [0], [0], [0])
        with pytest.raises(ValueError, match="11 bits"):
            enc([0], [2048], [0], [0])
        with pytest.raises(ValueError, match="non-decreasing"):
            enc([1, 2], [0, 0], [5, 4], [0, 0])
        with pytest.raises(ValueError, match="non-decreasing"):
            enc([1], [0], [-1], [0])
        with pytest.raises(ValueError, match="5 bits"):
            enc([], [], [], [], triggers=[[0, 32, 1]])
        with pytest.raises(ValueError, match="non-decreasing"):
            enc([], [], [], [], triggers=[[5, 1, 1], [4, 1, 0]])
        assert len(enc([2047], [2047], [0], [1], triggers=[[0, 31, 1]])) == 3
    with pytest.raises(ValueError, match="version 2"):
        r.encode_dat([1 << 14], [0], [0], [0])
    with pytest.raises(ValueError, match="version 2"):
        r.encode_dat([0], [1 << 14], [0], [0])
    with pytest.raises(ValueError, match="version 1"):
        r.encode_dat([512], [0], [0], [0], version=1)
    with pytest.raises(ValueError, match="version 1"):
        r.encode_dat([0], [256], [0], [0], version=1)
    with pytest.raises(ValueError, match="32 bits"):
        r.encode_dat([0], [0], [1 << 32], [0])
    with pytest.raises(ValueError, match="non-decreasing"):
        r.encode_dat([0, 0], [0, 0], [2, 1], [0, 0])
    with pytest.raises(ValueError, match="non-decreasing"):
        r.encode_dat([0], [0], [-1], [0])
    assert r.encode_dat([511], [255], [(1 << 32) - 1], [1], version=1).tolist() == [[(1 << 32) - 1, 0x3FFFF]]


def write(path, header, payload=b""):
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + payload)
    return str(path)


def test_evt21_endianness_rule_and_its_override(tmp_path):
    from event_based_bos_amd import recordings as r

    cases = (("% evt 2.1\n% end\n", True), ("% format EVT21;height=4;width=6\n% end\n", True),
             ("% evt 2.1\n% format EVT21;endianness=little;height=4;width=6\n% end\n", False),
             ("% format EVT21;height=4;width=6;endianness=little\n% end\n", False),
             ("% format EVT21;endianness=big;height=4;width=6\n% end\n", True))
    for text, want in cases:
        h = r.read_header(write(tmp_path / "a.raw", text))
        assert h.format == "EVT21" and r.half_swapped_of(h) is want, text
        assert r.half_swapped_of(h, False) is False and r.half_swapped_of(h, True) is True
    # the written file declares the plain order and reads back word for word
    path = str(tmp_path / "w.raw")
    r.write_raw_file(path, ref.EVT21_EXAMPLE_WORDS, 1280, 720, "EVT21")
    h = r.read_header(path)
    assert (h.format, h.width, h.height, r.half_swapped_of(h)) == ("EVT21", 1280, 720, False)
    assert np.fromfile(path, dtype="<u8", offset=h.payload_offset).tolist() == ref.EVT21_EXAMPLE_WORDS
    r.write_raw_file(path, ref.EVT2_EXAMPLE_WORDS, 640, 480, "EVT2")
    h = r.read_header(path)
    assert (h.format, h.width, h.height, h.fields["evt"]) == ("EVT2", 640, 480, "2.0")
    assert np.fromfile(path, dtype="<u4", offset=h.payload_offset).tolist() == ref.EVT2_EXAMPLE_WORDS
    with pytest.raises(ValueError):
        r.write_raw_file(path, [], 4, 4, "DAT")


def test_dat_headers(tmp_path):
    from event_based_bos_amd import recordings as r

    records = np.array(ref.DAT2_EXAMPLE_RECORDS, dtype="<u4")
    path = str(tmp_path / "a_td.dat")
    r.write_dat_file(path, records, 640, 480)
    h = r.read_header(path)
    assert (h.format, h.width, h.height, r.dat_version(h)) == ("DAT", 640, 480, 2)
    assert h.payload_offset == os.path.getsize(path) - records.nbytes
    assert np.fromfile(path, dtype="<u4", offset=h.payload_offset).reshape(-1, 2).tolist() == rows(ref.DAT2_EXAMPLE_RECORDS)
    r.write_dat_file(path, ref.DAT1_EXAMPLE_RECORDS, 304, 240, version=1)
    assert r.dat_version(r.read_header(path)) == 1
    # without a header there are no type and size bytes either: the records begin at once, version 2
    r.write_dat_file(path, records, 640, 480, header=False)
    h = r.read_header(path)
    assert (h.format, h.width, h.payload_offset, r.dat_version(h)) == ("DAT", None, 0, 2) and os.path.getsize(path) == records.nbytes
    # an event size other than 8 is refused; so is a version that is not 1 or 2
    with pytest.raises(ValueError, match="event size 16"):
        r.read_header(write(tmp_path / "b.dat", "% Version 2\n% Height 4\n% Width 6\n", bytes([0x0C, 16]) + records.tobytes()))
    with pytest.raises(ValueError, match="version"):
        r.dat_version(r.read_header(write(tmp_path / "c.dat", "% Version 3\n", bytes([0x0C, 8]))))
    # `% format DAT` names the format whatever the suffix
    h = r.read_header(write(tmp_path / "d.raw", "% format DAT\n% Width 6\n% Height 4\n% end\n", bytes([0x0C, 8]) + records.tobytes()))
    assert (h.format, h.width, h.height) == ("DAT", 6, 4) and h.payload_offset == os.path.getsize(tmp_path / "d.raw") - records.nbytes


def test_decode_recording_checks_the_header_first(tmp_path):
    from event_based_bos_amd import recordings as r

    with pytest.raises(ValueError, match="no format"):
        r.decode_recording(write(tmp_path / "a.raw", "% geometry 640x480\n% end\n"))
    with pytest.raises(NotImplementedError, match="EVT4"):
        r.decode_recording(write(tmp_path / "b.raw", "% format EVT4;height=4;width=6\n% end\n"))
    for text in ("% evt 2.0\n% end\n", "% evt 2.1\n% end\n"):
        with pytest.raises(ValueError, match="geometry"):
            r.decode_recording(write(tmp_path / "c.raw", text))
    path = str(tmp_path / "d.dat")
    r.write_dat_file(path, ref.DAT2_EXAMPLE_RECORDS, 0, 0, header=False)
    with pytest.raises(ValueError, match="geometry"):
        r.decode_recording(path)
    with pytest.raises(ValueError, match="slab_words"):
        r.decode_recording(write(tmp_path / "e.raw", "% evt 2.0\n% geometry 640x480\n% end\n"), slab_words=0)


def test_a_payload_tail_is_dropped_with_a_warning(tmp_path, caplog):
    from event_based_bos_amd import recordings as r

    path = str(tmp_path / "w.raw")
    r.write_raw_file(path, ref.EVT21_EXAMPLE_WORDS, 1280, 720, "EVT21")
    h = r.read_header(path)
    with caplog.at_level(logging.WARNING):
        assert r._payload_items(path, h, 8, "words") == len(ref.EVT21_EXAMPLE_WORDS) and not caplog.records
        with open(path, "ab") as f:
            f.write(b"\x01\x02\x03")
        assert r._payload_items(path, h, 8, "words") == len(ref.EVT21_EXAMPLE_WORDS)
    assert any("last 3 bytes are dropped" in rec.getMessage() for rec in caplog.records)


def test_c_entries_refuse_before_any_hip_call(lib):
    """Host-only queries and the argument checks of scan, emit and the DAT decode: usable without a GPU, like the other entries."""
    C4, C8 = lib.ebos_evt2_chunk_words(4), lib.ebos_evt2_chunk_words(8)
    assert C4 >= 256 and C4 % 4 == 0 and C8 >= 256 and C8 % 2 == 0
    for wb in (0, 2, 3, 5, 16, -4):
        assert lib.ebos_evt2_chunk_words(wb) == 0 and lib.ebos_evt2_scratch_bytes(100, wb) == 0
    p = 0x1000
    cols = [p] * 7
    for wb, C in ((4, C4), (8, C8)):
        need = lib.ebos_evt2_scratch_bytes(10 * C + 37, wb)
        assert need > 0 and lib.ebos_evt2_scratch_bytes(0, wb) > 0 and lib.ebos_evt2_scratch_bytes(100 * C, wb) > need
        assert lib.ebos_evt2_scratch_bytes(-1, wb) == 0 and lib.ebos_evt2_scratch_bytes((1 << 30) + 1, wb) == 0
        assert lib.ebos_evt2_scan(None, 5, wb, 0, None, p, p, p, need, None) == -1 and lib.ebos_last_error() == b"ebos_evt2_scan: words is NULL"
        assert lib.ebos_evt2_scan(p, -1, wb, 0, None, p, p, p, need, None) == -1 and b"n_words -1 outside" in lib.ebos_last_error()
        assert lib.ebos_evt2_scan(p, (1 << 30) + 1, wb, 0, None, p, p, p, need, None) == -1 and b"outside" in lib.ebos_last_error()
        assert lib.ebos_evt2_scan(p, 5, wb, 0, None, None, p, p, need, None) == -1 and b"NULL carry_out / totals / scratch" in lib.ebos_last_error()
        assert lib.ebos_evt2_scan(p, 5, wb, 0, None, p, None, p, need, None) == -1 and lib.ebos_evt2_scan(p, 5, wb, 0, None, p, p, None, need, None) == -1
        for off in range(1, wb):
            assert lib.ebos_evt2_scan(p + off, 5, wb, 0, None, p, p, p, need, None) == -1
            assert lib.ebos_last_error() == b"ebos_evt2_scan: words is not %d-byte aligned" % wb
            assert lib.ebos_evt2_emit(p + off, 5, wb, 0, p, need, 0, 0, 0, 0, *cols, None) == -1
            assert lib.ebos_last_error() == b"ebos_evt2_emit: words is not %d-byte aligned" % wb
        assert lib.ebos_evt2_scan(p, 5, wb, 0, None, p, p, p + 4, need, None) == -1 and b"scratch is not 8-byte aligned" in lib.ebos_last_error()
        assert lib.ebos_evt2_scan(p, 10 * C + 37, wb, 0, None, p, p, p, need - 1, None) == -4 and b"scratch too small" in lib.ebos_last_error()
        assert lib.ebos_evt2_emit(None, 5, wb, 0, p, need, 0, 0, 0, 0, *cols, None) == -1 and lib.ebos_last_error() == b"ebos_evt2_emit: words is NULL"
        assert lib.ebos_evt2_emit(p, 5, wb, 0, None, need, 0, 0, 0, 0, *cols, None) == -1
        assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, -1, 0, 0, 0, *cols, None) == -1 and b"negative" in lib.ebos_last_error()
        assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, 0, 0, 0, -1, *cols, None) == -1 and b"negative" in lib.ebos_last_error()
        # a capacity below the totals is refused before anything is written
        assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, 7, 0, 6, 0, *cols, None) == -1
        assert lib.ebos_last_error() == b"ebos_evt2_emit: event capacity 6 below the slab's 7 events"
        assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, 7, 2, 7, 1, *cols, None) == -1
        assert lib.ebos_last_error() == b"ebos_evt2_emit: trigger capacity 1 below the slab's 2 triggers"
        for k in range(4):
            holed = list(cols)
            holed[k] = None
            assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, 7, 0, 7, 0, *holed, None) == -1 and b"NULL event column" in lib.ebos_last_error()
        for k in range(4, 7):
            holed = list(cols)
            holed[k] = None
            assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, 0, 2, 0, 2, *holed, None) == -1 and b"NULL trigger column" in lib.ebos_last_error()
        assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, 1, 0, 1, 0, p + 1, p, p, p, p, p, p, None) == -1 and b"misaligned" in lib.ebos_last_error()
        assert lib.ebos_evt2_emit(p, 5, wb, 0, p, need, 1, 0, 1, 0, p, p, p + 4, p, p, p, p, None) == -1 and b"misaligned" in lib.ebos_last_error()
        assert lib.ebos_evt2_emit(p, 10 * C + 37, wb, 0, p, need - 1, 0, 0, 0, 0, *cols, None) == -4
    for wb in (0, 2, 16):
        assert lib.ebos_evt2_scan(p, 5, wb, 0, None, p, p, p, 1 << 20, None) == -1 and b"word_bytes" in lib.ebos_last_error()
        assert lib.ebos_evt2_emit(p, 5, wb, 0, p, 1 << 20, 0, 0, 0, 0, *cols, None) == -1 and b"word_bytes" in lib.ebos_last_error()
    # the DAT decode
    assert lib.ebos_dat_decode(None, 5, 2, p, p, p, p, 5, None) == -1 and lib.ebos_last_error() == b"ebos_dat_decode: records is NULL"
    assert lib.ebos_dat_decode(p, -1, 2, p, p, p, p, 5, None) == -1 and lib.ebos_dat_decode(p, (1 << 30) + 1, 2, p, p, p, p, 1 << 31, None) == -1
    assert lib.ebos_dat_decode(p, 5, 3, p, p, p, p, 5, None) == -1 and b"version 3" in lib.ebos_last_error()
    assert lib.ebos_dat_decode(p, 5, 0, p, p, p, p, 5, None) == -1
    assert lib.ebos_dat_decode(p, 5, 2, p, p, p, p, 4, None) == -1 and lib.ebos_last_error() == b"ebos_dat_decode: capacity 4 below the 5 records"
    assert lib.ebos_dat_decode(p + 4, 5, 2, p, p, p, p, 5, None) == -1 and b"not 8-byte aligned" in lib.ebos_last_error()
    for k in range(4):
        holed = [p] * 4
        holed[k] = None
        assert lib.ebos_dat_decode(p, 5, 2, *holed, 5, None) == -1 and b"NULL column" in lib.ebos_last_error()
    assert lib.ebos_dat_decode(p, 5, 2, p + 1, p, p, p, 5, None) == -1 and b"misaligned" in lib.ebos_last_error()
    assert lib.ebos_dat_decode(p, 5, 2, p, p, p + 4, p, 5, None) == -1 and b"misaligned" in lib.ebos_last_error()
    assert lib.ebos_dat_decode(None, 0, 2, None, None, None, None, 0, None) == 0          # nothing to do: no launch


def test_state_struct_layout_matches_the_ctypes_mirror(tmp_path):
    from event_based_bos_amd import _hip

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in _hip.Evt2State._fields_]
    hdr = open(os.path.join(ROOT, "include", "ebos_hip.h")).read()
    body = hdr[hdr.index("typedef struct ebos_evt2_state {"):hdr.index("} ebos_evt2_state;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split("{", 1)[1].split(";"):
        declared += re.findall(r"[*\s,]([A-Za-z_][A-Za-z0-9_]*)\s*(?=,|$)", stmt.strip())
    assert declared == fields == ["has_th", "th", "loops"]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ebos_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(ebos_evt2_state));']
    lines += [f'  printf("%zu\\n", offsetof(ebos_evt2_state, {f}));' for f in fields]
    src.write_text("\n".join(lines + ['  return 0;', '}']) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_hip.Evt2State)] + [getattr(_hip.Evt2State, f).offset for f in fields]
    assert ctypes.sizeof(_hip.Evt2State) == 16


def test_the_unit_is_part_of_the_build():
    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import SOURCES

    assert "evt2.hip" in SOURCES and "evt3.hip" in SOURCES and _hip.ABI_VERSION == 2
    assert {"ebos_evt2_chunk_words", "ebos_evt2_scratch_bytes", "ebos_evt2_scan", "ebos_evt2_emit", "ebos_dat_decode"} <= set(_hip.SIGNATURES)
    assert "ebos_evt21_route" not in _hip.SIGNATURES              # one emit pass for EVT 2.1, no switch
    assert ebos.recordings.decode_recording and ebos.recordings.FORMATS == ("EVT2", "EVT21", "EVT3", "DAT")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_decode(tmp_path):
    import event_based_bos_amd as ebos

    r = ebos.recordings
    files = []
    for fmt, words in (("EVT2", ref.EVT2_EXAMPLE_WORDS), ("EVT21", ref.EVT21_EXAMPLE_WORDS)):
        files.append(str(tmp_path / (fmt + ".raw")))
        r.write_raw_file(files[-1], words, 1280, 720, fmt)
    files.append(str(tmp_path / "x_td.dat"))
    r.write_dat_file(files[-1], ref.DAT2_EXAMPLE_RECORDS, 1280, 720)
    for path in files:
        with pytest.raises(ebos.HipUnavailableError):
            ebos.RawEventStore(path)
        with pytest.raises(ebos.HipUnavailableError):
            r.decode_recording(path)
    with pytest.raises(ebos.HipUnavailableError):
        r.decode_evt2(np.array(ref.EVT2_EXAMPLE_WORDS, dtype=np.uint32))
    with pytest.raises(ebos.HipUnavailableError):
        r.decode_evt21(np.array(ref.EVT21_EXAMPLE_WORDS, dtype=np.uint64))
    with pytest.raises(ebos.HipUnavailableError):
        r.decode_dat(np.array(ref.DAT2_EXAMPLE_RECORDS, dtype=np.uint32))
    with pytest.raises(ebos.HipUnavailableError):
        r.evt2_scan(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ebos.HipUnavailableError):
        r.evt2_emit(torch.zeros(4, dtype=torch.int32), torch.zeros(8, dtype=torch.uint8), 0, 0, *[torch.zeros(0)] * 7)


# ---------------------------------------------------------------------------------------------------- the state algebra on the CPU
ALGEBRA_MAIN = r"""
// Reads streams (word size, words, cuts) and prints, per stream, the final state and the totals twice: folded word by word, and as
// `then` over the records of the parts between the cuts (folded from the left and from the right).
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "evt2_core.h"
using namespace ebos;
static evt2::Word classify(const std::vector<uint64_t>& w, size_t i, int wb) {
  return wb == 4 ? evt2::classify32((uint32_t)w[i]) : evt2::classify64(w[i]);
}
static void show(const ebos_evt2_state& s, long long ev, long long tr) {
  printf("%d %d %lld %lld %lld\n", s.has_th, s.th, (long long)s.loops, ev, tr);
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t head[3];
  while (fread(head, sizeof(int64_t), 3, f) == 3) {
    const int wb = (int)head[0];
    std::vector<uint64_t> words((size_t)head[1]);
    std::vector<int64_t> cuts((size_t)head[2]);
    if (fread(words.data(), 8, words.size(), f) != words.size()) return 3;
    if (fread(cuts.data(), 8, cuts.size(), f) != cuts.size()) return 3;
    ebos_evt2_state s = {0, 0, 0};
    long long ev = 0, tr = 0;
    for (size_t i = 0; i < words.size(); ++i) {
      evt2::Xf one = evt2::identity();
      evt2::fold_word(one, classify(words, i, wb));
      evt2::apply(s, one, ev, tr);
    }
    show(s, ev, tr);
    std::vector<evt2::Xf> parts;
    size_t at = 0;
    for (size_t c = 0; c <= cuts.size(); ++c) {
      const size_t end = c < cuts.size() ? (size_t)cuts[c] : words.size();
      evt2::Xf x = evt2::identity();
      for (; at < end; ++at) evt2::fold_word(x, classify(words, at, wb));
      parts.push_back(x);
    }
    evt2::Xf left = evt2::identity(), right = evt2::identity();
    for (size_t c = 0; c < parts.size(); ++c) left = evt2::then(left, parts[c]);
    for (size_t c = parts.size(); c-- > 0;) right = evt2::then(parts[c], right);
    ebos_evt2_state sl = {0, 0, 0}, sr = {0, 0, 0};
    long long evl = 0, trl = 0, evr = 0, trr = 0;
    evt2::apply(sl, left, evl, trl);
    evt2::apply(sr, right, evr, trr);
    show(sl, evl, trl);
    show(sr, evr, trr);
  }
  fclose(f);
  return 0;
}
"""


def algebra_streams():
    """(word_bytes, words, cuts): random streams with random cuts, and streams aimed at the seams."""
    rng = np.random.default_rng(11)
    TH, EV, TR = 0x8 << 28, 0x1 << 28, 0xA << 28
    streams = []
    for k in range(12):
        n = int(rng.integers(1, 400))
        words = ref.random_evt2_words(rng, n, p_time_high=[0.0, 0.02, 0.2, 0.6][k % 4])
        cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 12))))       # (repeated cuts: empty parts)
        streams.append((4, words, cuts))
        words = ref.random_evt21_words(rng, n, p_time_high=[0.0, 0.02, 0.2, 0.6][k % 4])
        streams.append((8, words, cuts))
    top = (1 << 28) - 1
    aimed = [
        ([EV, TR, TH | 5, EV, EV, TH | 6, TR, EV], [2, 3, 5, 6]),          # TIME_HIGH as the first and as the last word of a part
        ([EV, EV, TR, EV], [1, 3]),                                          # no TIME_HIGH at all
        ([TH | 9, EV, EV, TR, EV, EV, TH | 9], [1, 3, 5]),                   # parts with no TIME_HIGH between parts that have one
        ([TH | top, EV, TH | 0, EV], [2]),                                   # a wrap exactly at a cut
        ([TH | top, TH | 0, TH | top, TH | 0, EV], [1, 2, 3]),               # a wrap at every cut
        ([TH | (top - 1), EV, TH | 9, EV], [2]),                             # prev - v = 2^28 - 11: the smallest fall that wraps
        ([TH | (top - 1), EV, TH | 10, EV], [2]),                            # prev - v = 2^28 - 12: no wrap
        ([TH | (top - 1), EV, TH | 10, EV], []),
        ([EV, TH | top, TH | 0, TH | top, TH | 0], [1]),                     # two wraps inside one part
    ]
    for words, cuts in aimed:
        streams.append((4, np.array(words, dtype=np.uint32), np.array(cuts, dtype=np.int64)))
        wide = [(((w >> 28) << 60) | ((w & top) << 32) | 0x5) for w in words]
        streams.append((8, np.array(wide, dtype=np.uint64), np.array(cuts, dtype=np.int64)))
    return streams


def test_state_algebra_on_the_cpu(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = tmp_path / "algebra.cpp"
    src.write_text(ALGEBRA_MAIN)
    exe = tmp_path / "algebra"
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "event_based_bos_amd", "csrc"),
            str(src), "-o", str(exe)]
    r = subprocess.run(base[:5] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[5:], capture_output=True, text=True)
    if r.returncode != 0:                                   # a compiler without the sanitizers' runtimes
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    streams = algebra_streams()
    data = tmp_path / "streams.bin"
    with open(data, "wb") as f:
        for wb, words, cuts in streams:
            f.write(struct.pack("<3q", wb, len(words), len(cuts)))
            f.write(np.asarray(words).astype("<u8").tobytes() + np.asarray(cuts).astype("<i8").tobytes())
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == 3 * len(streams)
    wraps = 0
    for k, (wb, words, cuts) in enumerate(streams):
        e, t, s = (ref.decode_evt2 if wb == 4 else ref.decode_evt21)(words)
        want = [s["has_th"], s["th"], s["loops"], len(e), len(t)]
        assert lines[3 * k] == want, (k, "word by word")
        assert lines[3 * k + 1] == want, (k, "then, from the left")
        assert lines[3 * k + 2] == want, (k, "then, from the right")
        wraps += s["loops"]
    assert wraps > 20       # the streams do wrap
