"""A sequential, word-by-word restatement of the EVT 3.0 rules this build decodes (the table of include/ebos_hip.h), in plain
Python: the yardstick of tests/test_evt3.py and tests/test_gpu_evt3.py.  It shares no code with the kernel or with the package's
encoder.  Neither OpenEB nor a camera file is part of this repository: the rules are restated, not checked against OpenEB."""
import numpy as np

TIME_HIGH, TIME_LOW, ADDR_Y, ADDR_X, VECT_BASE_X, VECT_12, VECT_8, EXT_TRIGGER = 0x8, 0x6, 0x0, 0x2, 0x3, 0x4, 0x5, 0xA

# the worked example of the format's description: words, events (x, y, t, p), triggers (t, value, id)
EXAMPLE_WORDS = [0x8001, 0x6010, 0x0005, 0x2803, 0x3064, 0x4805, 0x5081, 0x6FFF, 0xA101, 0x8002, 0x2003]
EXAMPLE_EVENTS = [(3, 5, 4112, 1), (100, 5, 4112, 0), (102, 5, 4112, 0), (111, 5, 4112, 0), (112, 5, 4112, 0), (119, 5, 4112, 0),
                  (3, 5, 8192, 0)]
EXAMPLE_TRIGGERS = [(8191, 1, 1)]

START = dict(has_th=0, th=0, tl=0, y=0, bx=0, pol=0, loops=0)


def decode(words, state=None):
    """(events int64 [n, 4] = (x, y, t, p), triggers int64 [m, 3] = (t, value, id), the final state) of ``words`` decoded one after
    the other from ``state`` (default: all zero).  ``bx`` is reported modulo 2^16 and x as the int16 of that bit pattern."""
    s = dict(START if state is None else state)
    events, triggers = [], []
    for w in np.asarray(words, dtype=np.uint16).tolist():
        kind, v = w >> 12, w & 0xFFF
        if kind == TIME_HIGH:
            if s["has_th"] and s["th"] > v and s["th"] - v >= 4085:
                s["loops"] += 1
            s["th"], s["tl"], s["has_th"] = v, 0, 1
            continue
        if not s["has_th"]:
            continue          # before the first TIME_HIGH a word emits nothing and sets nothing
        t = (s["loops"] << 24) | (s["th"] << 12) | s["tl"]
        if kind == TIME_LOW:
            s["tl"] = v
        elif kind == ADDR_Y:
            s["y"] = v & 0x7FF
        elif kind == ADDR_X:
            events.append((v & 0x7FF, s["y"], t, v >> 11))
        elif kind == VECT_BASE_X:
            s["bx"], s["pol"] = v & 0x7FF, v >> 11
        elif kind in (VECT_12, VECT_8):
            width = 12 if kind == VECT_12 else 8
            for b in range(width):
                if (v >> b) & 1:
                    x = (s["bx"] + b) & 0xFFFF
                    events.append((x - 0x10000 if x >= 0x8000 else x, s["y"], t, s["pol"]))
            s["bx"] = (s["bx"] + width) & 0xFFFF
        elif kind == EXT_TRIGGER:
            triggers.append((t, v & 1, v >> 8))
    return (np.array(events, dtype=np.int64).reshape(-1, 4), np.array(triggers, dtype=np.int64).reshape(-1, 3), s)


def random_words(rng, n, p_time_high=0.08):
    """``n`` random words over all sixteen types (the ignored ones included); TIME_HIGH values mostly step forward by a little so
    that wraps happen, with an occasional jump anywhere."""
    kinds = rng.choice(16, size=n, p=_kind_weights(p_time_high))
    v = rng.integers(0, 4096, size=n)
    words = (kinds.astype(np.int64) << 12) | v
    th = int(rng.integers(0, 4096))
    for i in np.nonzero(kinds == TIME_HIGH)[0]:
        th = int(rng.integers(0, 4096)) if rng.random() < 0.1 else (th + int(rng.integers(0, 9))) & 0xFFF
        words[i] = (TIME_HIGH << 12) | th
    return words.astype(np.uint16)


def _kind_weights(p_time_high):
    w = np.full(16, 0.01)
    w[[TIME_LOW, ADDR_Y, ADDR_X, VECT_BASE_X, VECT_12, VECT_8, EXT_TRIGGER]] = [0.1, 0.1, 0.2, 0.1, 0.15, 0.1, 0.03]
    w[TIME_HIGH] = 0.0
    w = w / w.sum() * (1.0 - p_time_high)
    w[TIME_HIGH] = p_time_high
    return w
