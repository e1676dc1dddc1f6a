"""A sequential, word-by-word restatement of the EVT 2.0, EVT 2.1 and DAT rules this build decodes (the table of
include/ebos_hip.h), in plain Python: the yardstick of tests/test_recordings.py and tests/test_gpu_recordings.py.  It shares no code
with the kernels or with the package's encoders.  Neither OpenEB nor a camera file is part of this repository: the rules are
restated from the format documentation, not checked against OpenEB."""
import numpy as np

TIME_HIGH, CD_OFF, CD_ON, EXT_TRIGGER = 0x8, 0x0, 0x1, 0xA
TH_MAX = (1 << 28) - 1
WRAP_FALL = (1 << 28) - 11

START = dict(has_th=0, th=0, loops=0)

# worked examples, every field placed by hand: words, events (x, y, t, p), triggers (t, value, id)
EVT2_EXAMPLE_WORDS = [
    0x10000C05,   # CD_ON before the first TIME_HIGH: ignored
    0x80000001,   # TIME_HIGH 1
    0x11401807,   # CD_ON   ts 5   x 3     y 7
    0x0FE7FACF,   # CD_OFF  ts 63  x 1279  y 719
    0xA2800301,   # EXT_TRIGGER ts 10, id 3, value 1
    0xE0001234,   # OTHERS: ignored
    0xF0001234,   # CONTINUED: ignored
    0x80000002,   # TIME_HIGH 2
    0x10000000,   # CD_ON   ts 0   x 0     y 0
]
EVT2_EXAMPLE_EVENTS = [(3, 7, 69, 1), (1279, 719, 127, 0), (0, 0, 128, 1)]
EVT2_EXAMPLE_TRIGGERS = [(74, 1, 3)]

EVT21_EXAMPLE_WORDS = [
    0x10000007FFFFFFFF,   # EVT_POS before the first TIME_HIGH: ignored
    0x8000000100000000,   # TIME_HIGH 1
    0x1143000780000005,   # EVT_POS ts 5  bx 96    y 7  valid bits 0, 2, 31
    0x003FF80000000003,   # EVT_NEG ts 0  bx 2047  y 0  valid bits 0, 1
    0xA280030100000000,   # EXT_TRIGGER ts 10, id 3, value 1
    0x8000000200000000,   # TIME_HIGH 2
    0x0040000100000000,   # EVT_NEG ts 1  bx 0     y 1  valid 0: nothing
    0x3000000000000001,   # an unlisted type: ignored
]
EVT21_EXAMPLE_EVENTS = [(96, 7, 69, 1), (98, 7, 69, 1), (127, 7, 69, 1), (2047, 0, 64, 0), (2048, 0, 64, 0)]
EVT21_EXAMPLE_TRIGGERS = [(74, 1, 3)]

DAT2_EXAMPLE_RECORDS = [(100, 0x10024005), (4000000000, 0x0FFFFFFF)]
DAT2_EXAMPLE_EVENTS = [(5, 9, 100, 1), (16383, 16383, 4000000000, 0)]
DAT1_EXAMPLE_RECORDS = [(7, 0x0003912C), (8, 0xFFFC0000)]
DAT1_EXAMPLE_EVENTS = [(300, 200, 7, 1), (0, 0, 8, 0)]


def _time_high(s, v):
    if s["has_th"] and s["th"] > v and s["th"] - v >= WRAP_FALL:
        s["loops"] += 1
    s["th"], s["has_th"] = v, 1


def _arrays(events, triggers):
    return np.array(events, dtype=np.int64).reshape(-1, 4), np.array(triggers, dtype=np.int64).reshape(-1, 3)


def decode_evt2(words, state=None):
    """(events int64 [n, 4] = (x, y, t, p), triggers int64 [m, 3] = (t, value, id), the final state) of uint32 ``words`` decoded
    one after the other from ``state`` (default: all zero)."""
    s = dict(START if state is None else state)
    events, triggers = [], []
    for w in np.asarray(words, dtype=np.uint32).tolist():
        kind = w >> 28
        if kind == TIME_HIGH:
            _time_high(s, w & 0x0FFFFFFF)
            continue
        if not s["has_th"]:
            continue
        t = (s["loops"] << 34) | (s["th"] << 6) | ((w >> 22) & 0x3F)
        if kind in (CD_OFF, CD_ON):
            events.append(((w >> 11) & 0x7FF, w & 0x7FF, t, kind))
        elif kind == EXT_TRIGGER:
            triggers.append((t, w & 1, (w >> 8) & 0x1F))
    return _arrays(events, triggers) + (s,)


def decode_evt21(words, state=None, half_swapped=False):
    """The same for uint64 ``words``; ``half_swapped``: the two 32-bit halves of every word are exchanged first."""
    s = dict(START if state is None else state)
    events, triggers = [], []
    for w in np.asarray(words, dtype=np.uint64).tolist():
        if half_swapped:
            w = ((w << 32) | (w >> 32)) & 0xFFFFFFFFFFFFFFFF
        kind = w >> 60
        if kind == TIME_HIGH:
            _time_high(s, (w >> 32) & 0x0FFFFFFF)
            continue
        if not s["has_th"]:
            continue
        t = (s["loops"] << 34) | (s["th"] << 6) | ((w >> 54) & 0x3F)
        if kind in (CD_OFF, CD_ON):
            bx, y = (w >> 43) & 0x7FF, (w >> 32) & 0x7FF
            for b in range(32):
                if (w >> b) & 1:
                    events.append((bx + b, y, t, kind))
        elif kind == EXT_TRIGGER:
            triggers.append((t, (w >> 32) & 1, (w >> 40) & 0x1F))
    return _arrays(events, triggers) + (s,)


def decode_dat(records, version=2):
    """events int64 [n, 4] = (x, y, t, p) of the records uint32 [n, 2] = (ts, data)."""
    events = []
    for ts, data in np.asarray(records, dtype=np.uint32).reshape(-1, 2).tolist():
        if version == 2:
            events.append((data & 0x3FFF, (data >> 14) & 0x3FFF, ts, (data >> 28) & 1))
        else:
            events.append((data & 0x1FF, (data >> 9) & 0xFF, ts, (data >> 17) & 1))
    return np.array(events, dtype=np.int64).reshape(-1, 4)


def _kinds(rng, n, p_time_high):
    w = np.full(16, 0.02)
    w[[CD_OFF, CD_ON, EXT_TRIGGER]] = [0.35, 0.35, 0.04]
    w[TIME_HIGH] = 0.0
    w = w / w.sum() * (1.0 - p_time_high)
    w[TIME_HIGH] = p_time_high
    return rng.choice(16, size=n, p=w)


def _time_high_values(rng, n):
    """TIME_HIGH values that wrap often: a value within 6 of the top is followed by one within 6 of zero, so the fall lies on both
    sides of the threshold; otherwise a small step forward or a jump anywhere."""
    out, th, top = np.zeros(n, np.int64), int(rng.integers(0, TH_MAX)), False
    for i in range(n):
        r = rng.random()
        if top:
            th, top = int(rng.integers(0, 7)), False
        elif r < 0.3:
            th, top = TH_MAX - int(rng.integers(0, 7)), True
        elif r < 0.4:
            th = int(rng.integers(0, TH_MAX + 1))
        else:
            th = (th + int(rng.integers(0, 5))) & TH_MAX
        out[i] = th
    return out


def random_evt2_words(rng, n, p_time_high=0.05):
    """``n`` random EVT 2.0 words over all sixteen types, the ignored ones included."""
    kinds = _kinds(rng, n, p_time_high)
    words = (kinds.astype(np.int64) << 28) | rng.integers(0, 1 << 28, size=n)
    at = np.nonzero(kinds == TIME_HIGH)[0]
    words[at] = (TIME_HIGH << 28) | _time_high_values(rng, len(at))
    return words.astype(np.uint32)


def random_evt21_words(rng, n, p_time_high=0.05):
    """``n`` random EVT 2.1 words over all sixteen types; the masks are empty, sparse, dense or full."""
    kinds = _kinds(rng, n, p_time_high).astype(np.uint64)
    upper = rng.integers(0, 1 << 28, size=n).astype(np.uint64)
    valid = rng.integers(0, 1 << 32, size=n).astype(np.uint64)
    style = rng.integers(0, 4, size=n)
    valid = np.where(style == 0, valid & rng.integers(0, 1 << 32, size=n).astype(np.uint64) & rng.integers(0, 1 << 32, size=n).astype(np.uint64), valid)
    valid = np.where(style == 1, np.uint64(1) << rng.integers(0, 32, size=n).astype(np.uint64), valid)
    valid = np.where((style == 2) & (rng.random(n) < 0.3), np.uint64(0), valid)
    valid = np.where((style == 3) & (rng.random(n) < 0.3), np.uint64(0xFFFFFFFF), valid)
    words = (kinds << np.uint64(60)) | (upper << np.uint64(32)) | valid
    at = np.nonzero(kinds == TIME_HIGH)[0]
    words[at] = (np.uint64(TIME_HIGH) << np.uint64(60)) | (_time_high_values(rng, len(at)).astype(np.uint64) << np.uint64(32)) | valid[at]
    return words
