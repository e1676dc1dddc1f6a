"""EVT 3.0 ``.raw`` recordings, the host side: the sequential restatement of the word rules (tests/_evt3_ref.py) on the worked
example, the package's encoder read back through it, the header, and the C entries' refusals -- nothing here needs a GPU."""
import ctypes
import logging
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _evt3_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


def test_worked_example_through_the_restatement():
    events, triggers, state = ref.decode(ref.EXAMPLE_WORDS)
    assert events.tolist() == [list(e) for e in ref.EXAMPLE_EVENTS]
    assert triggers.tolist() == [list(t) for t in ref.EXAMPLE_TRIGGERS]
    assert state == dict(has_th=1, th=2, tl=0, y=5, bx=120, pol=0, loops=0)
    # every word before the first TIME_HIGH is ignored altogether: the ADDR_Y there does not count
    events, triggers, state = ref.decode([0x0007, 0x2803, 0xA101, 0x6010] + ref.EXAMPLE_WORDS[:1] + [0x2803])
    assert events.tolist() == [[3, 0, 4096, 1]] and len(triggers) == 0
    # a wrap needs a fall of at least 4085; a smaller step backwards is kept as it is
    assert ref.decode([0x8FFF, 0x8000, 0x2001])[0].tolist() == [[1, 0, 1 << 24, 0]]
    assert ref.decode([0x8FF5, 0x8000, 0x2001])[0].tolist() == [[1, 0, 1 << 24, 0]]
    assert ref.decode([0x8FF4, 0x8000, 0x2001])[0].tolist() == [[1, 0, 0, 0]]


def recording(seed, n=4000, t0=0):
    """Columns with bursts of equal time, runs of ascending x on one row, wraps of the 24-bit time and a 5 s silent gap."""
    rng = np.random.default_rng(seed)
    t = t0 + np.cumsum(rng.choice([0, 0, 0, 1, 3, 700, 5000], size=n))
    t[n // 2:] += 5_000_000                         # a silent gap of 5 s
    t[n // 3:] += 3 * (1 << 24)                     # three wraps at once
    y = np.repeat(rng.integers(0, 720, size=n // 6 + 1), 6)[:n]
    x = rng.integers(0, 1280, size=n)
    for i in range(0, n - 8, 8):
        lo = int(x[i]) % 1200
        x[i:i + 6] = np.sort(rng.choice(np.arange(lo, lo + 40), 6, replace=False))
    p = np.repeat(rng.integers(0, 2, size=n // 3 + 1), 3)[:n]
    m = 23
    triggers = np.stack([np.sort(rng.integers(int(t[0]), int(t[-1]) + 100, size=m)), rng.integers(0, 16, size=m),
                         rng.integers(0, 2, size=m)], 1)
    return x, y, t, p, triggers


@pytest.mark.parametrize("t0", [0, (1 << 31) + 5], ids=["from0", "past2^31"])
@pytest.mark.parametrize("vectorize", [True, False])
def test_encoder_round_trip_through_the_restatement(t0, vectorize):
    from event_based_bos_amd import evt3

    x, y, t, p, triggers = recording(3, t0=t0)
    assert t[-1] - t[0] > 3 * (1 << 24) and (t0 == 0 or t[0] > 1 << 31)
    words = evt3.encode_evt3(x, y, t, p, triggers, vectorize=vectorize)
    assert words.dtype == np.uint16
    kinds = np.bincount(words >> 12, minlength=16)
    assert (kinds[ref.VECT_12] > 0 and kinds[ref.VECT_8] > 0 and kinds[ref.VECT_BASE_X] > 0) == vectorize
    high = (words[words >> 12 == ref.TIME_HIGH] & 0xFFF).astype(np.int64)
    assert np.all((np.diff(high) % 4096) <= 8)      # consecutive TIME_HIGH words never differ by more than 8 ticks
    events, trig, _ = ref.decode(words)
    assert np.array_equal(events[:, 0], x) and np.array_equal(events[:, 1], y)
    assert np.array_equal(events[:, 2], t) and np.array_equal(events[:, 3], p)
    assert np.array_equal(trig[:, [0, 2, 1]], triggers)


def test_encoder_refuses_what_the_format_cannot_hold():
    from event_based_bos_amd import evt3

    assert len(evt3.encode_evt3([], [], [], [])) == 0
    with pytest.raises(ValueError):
        evt3.encode_evt3([2048], [0], [0], [0])
    with pytest.raises(ValueError):
        evt3.encode_evt3([1, 2], [0, 0], [5, 4], [0, 0])
    with pytest.raises(ValueError):
        evt3.encode_evt3([], [], [], [], triggers=[[0, 16, 1]])


def write(path, header, payload=b""):
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + payload)
    return str(path)


def test_header_variants(tmp_path):
    from event_based_bos_amd import evt3

    words = np.array(ref.EXAMPLE_WORDS, dtype="<u2").tobytes()
    h = evt3.read_raw_header(write(tmp_path / "a.raw", "% date 2024-01-01 10:00:00\n% evt 3.0\n% format EVT3;height=720;width=1280\n% end\n", words))
    assert (h.format, h.width, h.height) == ("EVT3", 1280, 720) and h.fields["date"] == "2024-01-01 10:00:00"
    assert h.payload_offset == os.path.getsize(tmp_path / "a.raw") - len(words)
    # without `% end` the header ends at the first byte that is not '%'; the geometry line serves as well
    h = evt3.read_raw_header(write(tmp_path / "b.raw", "% evt 3.0\n% geometry 640x480\n", words))
    assert (h.format, h.width, h.height) == ("EVT3", 640, 480) and h.payload_offset == len("% evt 3.0\n% geometry 640x480\n")
    # `% end` ends the header even if more '%' lines follow: 0x2525 0x2525 ... would be payload
    h = evt3.read_raw_header(write(tmp_path / "c.raw", "% format EVT3;height=4;width=6\n% end\n", b"%%%%\n\n"))
    assert h.payload_offset == len("% format EVT3;height=4;width=6\n% end\n") and (h.width, h.height) == (6, 4)
    # another format is named in the refusal; a missing geometry is a ValueError unless the caller supplies one
    for text, name in (("% evt 2.0\n% geometry 640x480\n% end\n", "EVT2"), ("% evt 2.1\n% end\n", "EVT21"),
                       ("% format EVT21;height=4;width=6\n% end\n", "EVT21"), ("% format DAT\n% end\n", "DAT")):
        with pytest.raises(NotImplementedError, match=name):
            evt3.decode_raw_file(write(tmp_path / "d.raw", text, words))
    bare = write(tmp_path / "e.raw", "% evt 3.0\n% end\n", words)
    with pytest.raises(ValueError, match="geometry"):
        evt3.decode_raw_file(bare)
    assert evt3.read_raw_header(bare).width is None
    h = evt3._checked_header(bare, (720, 1280))
    assert (h.width, h.height) == (1280, 720)
    with pytest.raises(ValueError, match="no format"):
        evt3.decode_raw_file(write(tmp_path / "f.raw", "% geometry 640x480\n% end\n", words))


def test_written_file_reads_back_and_an_odd_trailing_byte_is_dropped(tmp_path, caplog):
    from event_based_bos_amd import evt3

    path = str(tmp_path / "w.raw")
    evt3.write_raw_file(path, ref.EXAMPLE_WORDS, 1280, 720)
    h = evt3.read_raw_header(path)
    assert (h.format, h.width, h.height) == ("EVT3", 1280, 720)
    assert np.fromfile(path, dtype="<u2", offset=h.payload_offset).tolist() == ref.EXAMPLE_WORDS
    with caplog.at_level(logging.WARNING):
        assert evt3.raw_word_count(path, h) == len(ref.EXAMPLE_WORDS) and not caplog.records
        with open(path, "ab") as f:
            f.write(b"\x01")
        assert evt3.raw_word_count(path, h) == len(ref.EXAMPLE_WORDS)
    assert any("odd length" in r.getMessage() for r in caplog.records)


def test_c_entries_refuse_before_any_hip_call(lib):
    """Host-only queries and the argument checks of scan and emit: usable without a GPU, like the other entries."""
    C = lib.ebos_evt3_chunk_words()
    assert C >= 256 and C % 8 == 0
    need = lib.ebos_evt3_scratch_bytes(10 * C + 37)
    assert need > 0 and lib.ebos_evt3_scratch_bytes(0) > 0 and lib.ebos_evt3_scratch_bytes(100 * C) > need
    assert lib.ebos_evt3_scratch_bytes(-1) == 0 and lib.ebos_evt3_scratch_bytes((1 << 30) + 1) == 0
    p = 0x1000
    assert lib.ebos_evt3_scan(None, 5, None, p, p, p, need, None) == -1 and lib.ebos_last_error() == b"ebos_evt3_scan: words is NULL"
    assert lib.ebos_evt3_scan(p, -1, None, p, p, p, need, None) == -1 and b"n_words -1 outside" in lib.ebos_last_error()
    assert lib.ebos_evt3_scan(p, 5, None, None, p, p, need, None) == -1 and b"NULL carry_out / totals / scratch" in lib.ebos_last_error()
    assert lib.ebos_evt3_scan(p, 5, None, p, None, p, need, None) == -1 and lib.ebos_evt3_scan(p, 5, None, p, p, None, need, None) == -1
    assert lib.ebos_evt3_scan(p + 1, 5, None, p, p, p, need, None) == -1 and b"not 2-byte aligned" in lib.ebos_last_error()
    assert lib.ebos_evt3_scan(p, 10 * C + 37, None, p, p, p, need - 1, None) == -4 and b"scratch too small" in lib.ebos_last_error()
    cols = [p] * 7
    assert lib.ebos_evt3_emit(None, 5, p, need, 0, 0, 0, 0, *cols, None) == -1 and lib.ebos_last_error() == b"ebos_evt3_emit: words is NULL"
    assert lib.ebos_evt3_emit(p, 5, None, need, 0, 0, 0, 0, *cols, None) == -1
    assert lib.ebos_evt3_emit(p, 5, p, need, -1, 0, 0, 0, *cols, None) == -1 and b"negative" in lib.ebos_last_error()
    # a capacity below the totals is refused before anything is written
    assert lib.ebos_evt3_emit(p, 5, p, need, 7, 0, 6, 0, *cols, None) == -1
    assert lib.ebos_last_error() == b"ebos_evt3_emit: event capacity 6 below the slab's 7 events"
    assert lib.ebos_evt3_emit(p, 5, p, need, 7, 2, 7, 1, *cols, None) == -1
    assert lib.ebos_last_error() == b"ebos_evt3_emit: trigger capacity 1 below the slab's 2 triggers"
    assert lib.ebos_evt3_emit(p, 5, p, need, 7, 0, 7, 0, p, None, p, p, p, p, p, None) == -1 and b"NULL event column" in lib.ebos_last_error()
    assert lib.ebos_evt3_emit(p, 5, p, need, 0, 2, 0, 2, p, p, p, p, None, p, p, None) == -1 and b"NULL trigger column" in lib.ebos_last_error()
    assert lib.ebos_evt3_emit(p, 10 * C + 37, p, need - 1, 0, 0, 0, 0, *cols, None) == -4


def test_state_struct_layout_matches_the_ctypes_mirror(tmp_path):
    from event_based_bos_amd import _hip

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in _hip.Evt3State._fields_]
    hdr = open(os.path.join(ROOT, "include", "ebos_hip.h")).read()
    body = hdr[hdr.index("typedef struct ebos_evt3_state {"):hdr.index("} ebos_evt3_state;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split("{", 1)[1].split(";"):
        declared += re.findall(r"[*\s,]([A-Za-z_][A-Za-z0-9_]*)\s*(?=,|$)", stmt.strip())
    assert declared == fields
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ebos_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(ebos_evt3_state));']
    lines += [f'  printf("%zu\\n", offsetof(ebos_evt3_state, {f}));' for f in fields]
    src.write_text("\n".join(lines + ['  return 0;', '}']) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_hip.Evt3State)] + [getattr(_hip.Evt3State, f).offset for f in fields]
    assert ctypes.sizeof(_hip.Evt3State) == 32


def test_the_unit_is_part_of_the_build():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import SOURCES

    assert "evt3.hip" in SOURCES and _hip.ABI_VERSION == 2
    assert {"ebos_evt3_chunk_words", "ebos_evt3_scratch_bytes", "ebos_evt3_scan", "ebos_evt3_emit"} <= set(_hip.SIGNATURES)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_decode(tmp_path):
    import event_based_bos_amd as ebos

    path = str(tmp_path / "x.raw")
    ebos.evt3.write_raw_file(path, ref.EXAMPLE_WORDS, 1280, 720)
    with pytest.raises(ebos.HipUnavailableError):
        ebos.RawEventStore(path)
    with pytest.raises(ebos.HipUnavailableError):
        ebos.evt3.decode_evt3(np.array(ref.EXAMPLE_WORDS, dtype=np.uint16))
    with pytest.raises(ebos.HipUnavailableError):
        ebos.evt3.decode_raw_file(path)
