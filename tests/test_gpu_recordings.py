"""The EVT 2.0, EVT 2.1 and DAT decode on the GPU (csrc/evt2.hip) against the sequential restatement of the word rules
(tests/_evt2_ref.py): every comparison is exact equality of integer arrays -- events, triggers and the carried state -- with the
streams aimed at the seams between the chunks of C = ebos_evt2_chunk_words(word size) words."""
import os

import numpy as np
import pytest
import torch

import _evt2_ref as ref

pytestmark = pytest.mark.gpu

TOP = (1 << 28) - 1


class Fmt:
    """One format's words: how to make them, and the two decoders."""

    def __init__(self, name):
        self.name = name
        self.wide = name == "EVT21"
        self.dtype = np.uint64 if self.wide else np.uint32

    def th(self, v):
        return (0x8 << 60) | (v << 32) if self.wide else (0x8 << 28) | v

    def ev(self, p=1, ts=0, x=0, y=0, valid=1):
        return (p << 60) | (ts << 54) | (x << 43) | (y << 32) | valid if self.wide else (p << 28) | (ts << 22) | (x << 11) | y

    def trig(self, ts=0, tid=0, value=1):
        return (0xA << 60) | (ts << 54) | (tid << 40) | (value << 32) if self.wide else (0xA << 28) | (ts << 22) | (tid << 8) | value

    def words(self, items):
        return np.array(items, dtype=self.dtype)

    def random(self, rng, n, p_time_high=0.05):
        return (ref.random_evt21_words if self.wide else ref.random_evt2_words)(rng, n, p_time_high)

    def want(self, words, state=None):
        return (ref.decode_evt21 if self.wide else ref.decode_evt2)(words, state)

    def slab(self, words, carry=None, half_swapped=False):
        from event_based_bos_amd import recordings

        if not self.wide:
            return recordings.decode_evt2(words, carry)
        return recordings.decode_evt21(words, carry, half_swapped=half_swapped)

    def decode(self, words, carry=None, half_swapped=False):
        """(events [n, 4], triggers [m, 3], state dict, the device carry) in the restatement's layout."""
        from event_based_bos_amd import recordings

        s = self.slab(np.asarray(words, dtype=self.dtype), carry, half_swapped)
        assert (s.x.dtype, s.y.dtype, s.t.dtype, s.p.dtype) == (torch.int16, torch.int16, torch.int64, torch.uint8)
        assert (s.trigger_t.dtype, s.trigger_value.dtype, s.trigger_id.dtype) == (torch.int64, torch.uint8, torch.uint8)
        events = torch.stack([c.to(torch.int64) for c in (s.x, s.y, s.t, s.p)], 1).cpu().numpy()
        triggers = torch.stack([c.to(torch.int64) for c in (s.trigger_t, s.trigger_value, s.trigger_id)], 1).cpu().numpy()
        return events, triggers, recordings.carry_to_dict(s.carry), s.carry

    def check(self, words, state=None):
        from event_based_bos_amd import recordings

        words = np.asarray(words, dtype=self.dtype)
        want_e, want_t, want_s = self.want(words, state)
        got_e, got_t, got_s, _ = self.decode(words, None if state is None else recordings.new_carry("cuda", state))
        assert got_e.shape == want_e.shape and np.array_equal(got_e, want_e)
        assert got_t.shape == want_t.shape and np.array_equal(got_t, want_t)
        assert got_s == want_s
        return want_e, want_t, want_s


FORMATS = [Fmt("EVT2"), Fmt("EVT21")]


@pytest.fixture(scope="module", params=FORMATS, ids=["evt2", "evt21-walk"])     # (the ids these cases have had: the emit pass is the lane walk)
def fmt(request):
    return request.param


@pytest.fixture(scope="module")
def C(fmt):
    from event_based_bos_amd import recordings

    c = recordings.chunk_words(fmt.name)
    assert c >= 256
    return c


def filler(fmt, rng, n):
    """Words without a TIME_HIGH: events, triggers and ignored types."""
    return fmt.random(rng, n, p_time_high=0.0)


def test_worked_example(fmt):
    words, events, triggers = ((ref.EVT21_EXAMPLE_WORDS, ref.EVT21_EXAMPLE_EVENTS, ref.EVT21_EXAMPLE_TRIGGERS) if fmt.wide else
                               (ref.EVT2_EXAMPLE_WORDS, ref.EVT2_EXAMPLE_EVENTS, ref.EVT2_EXAMPLE_TRIGGERS))
    e, t, s = fmt.check(words)
    assert e.tolist() == [list(v) for v in events] and t.tolist() == [list(v) for v in triggers] and s == dict(has_th=1, th=2, loops=0)


def test_random_stream_over_every_word_type(fmt, C):
    words = fmt.random(np.random.default_rng(1), 5 * C + 37)
    assert set((words >> np.array(60 if fmt.wide else 28, dtype=fmt.dtype)).tolist()) == set(range(16))
    e, t, s = fmt.check(words)
    assert len(e) > C and len(t) > 10 and s["loops"] > 0
    fmt.check(words[5:], dict(has_th=1, th=TOP - 2, loops=(1 << 25) + 2))      # from a carried state, t past 2^59


def test_lengths_around_a_chunk(fmt, C):
    rng = np.random.default_rng(7)
    stream = fmt.random(rng, 3 * C + 37, p_time_high=0.05)
    stream[0] = fmt.th(9)
    for n in (0, 1, C - 1, C, C + 1, 3 * C + 37):
        fmt.check(stream[:n])
        fmt.check(stream[1:][:n], dict(has_th=1, th=3, loops=7))


def test_time_high_at_the_last_and_at_the_first_word_of_a_chunk(fmt, C):
    rng = np.random.default_rng(2)
    for at in (C - 1, C):
        words = np.concatenate((fmt.words([fmt.th(5)]), filler(fmt, rng, 2 * C + 10)))
        words[at] = fmt.th(77)
        words[at - 1], words[at + 1] = fmt.ev(1, 3, 10, 20), fmt.ev(0, 4, 11, 21)
        e, _, s = fmt.check(words)
        assert s["th"] == 77 and [10, 20, (5 << 6) | 3, 1] in e.tolist() and [11, 21, (77 << 6) | 4, 0] in e.tolist()


def test_chunks_without_time_high_and_of_nothing_but_time_high(fmt, C):
    rng = np.random.default_rng(4)
    only_th = fmt.words([fmt.th(100 + k // 3) for k in range(C)])
    words = np.concatenate((fmt.words([fmt.th(1)]), filler(fmt, rng, C - 1), filler(fmt, rng, C), only_th, filler(fmt, rng, C // 2)))
    kinds = words >> np.array(60 if fmt.wide else 28, dtype=fmt.dtype)
    assert not np.any(kinds[C:2 * C] == ref.TIME_HIGH) and np.all(kinds[2 * C:3 * C] == ref.TIME_HIGH)
    fmt.check(words)
    e, t, s = fmt.check(np.concatenate((only_th, only_th)))          # no event at all
    assert len(e) == 0 and len(t) == 0 and s["has_th"] == 1


def test_first_time_high_in_the_third_chunk(fmt, C):
    rng = np.random.default_rng(5)
    words = np.concatenate((filler(fmt, rng, 2 * C + 100), fmt.words([fmt.th(77)]), filler(fmt, rng, C)))
    words[2 * C + 99] = fmt.ev(1, 1, 1, 1)                  # the last word before the first TIME_HIGH does not count
    words[2 * C + 101] = fmt.ev(0, 2, 2, 2)
    e, t, _ = fmt.check(words)
    assert e[0].tolist() == [2, 2, (77 << 6) | 2, 0] and 0 < len(e) and np.all(e[:, 2] >= 77 << 6) and np.all(t[:, 0] >= 77 << 6)


def test_no_time_high_at_all_gives_nothing(fmt, C):
    words = filler(fmt, np.random.default_rng(6), 3 * C + 5)
    e, t, s = fmt.check(words)
    assert len(e) == 0 and len(t) == 0 and s == ref.START


def test_wraps_at_a_seam_and_inside_a_chunk(fmt, C):
    rng = np.random.default_rng(3)
    base = np.concatenate((fmt.words([fmt.th(4000)]), filler(fmt, rng, 3 * C)))
    # a wrap exactly at a seam: prev = 2^28 - 1 ends chunk 0, v = 0 begins chunk 1
    words = base.copy()
    words[C - 1], words[C], words[C + 1] = fmt.th(TOP), fmt.th(0), fmt.ev(1, 7, 17, 18)
    e, _, s = fmt.check(words)
    assert s["loops"] == 1 and [17, 18, (1 << 34) | 7, 1] in e.tolist()
    # the smallest fall that wraps, and the backward step that is not a wrap: prev - v = 2^28 - 12
    for v, loops in ((9, 1), (10, 0)):
        words = base.copy()
        words[C - 1], words[C], words[C + 1] = fmt.th(TOP - 1), fmt.th(v), fmt.ev(1, 0, 17, 18)
        e, _, s = fmt.check(words)
        assert s["loops"] == loops and [17, 18, (loops << 34) | (v << 6), 1] in e.tolist()
    # two wraps inside one chunk
    words = base.copy()
    words[C + 10], words[C + 11], words[C + 500], words[C + 501] = fmt.th(TOP), fmt.th(3), fmt.th(TOP - 4), fmt.th(1)
    words[C + 502] = fmt.ev(0, 63, 1, 2)
    e, _, s = fmt.check(words)
    assert s["loops"] == 2 and [1, 2, (2 << 34) | (1 << 6) | 63, 0] in e.tolist()


def test_triggers_at_seams(fmt, C):
    rng = np.random.default_rng(8)
    words = np.concatenate((fmt.words([fmt.th(6)]), filler(fmt, rng, 3 * C)))
    for k, at in enumerate((C - 1, C, 2 * C - 1, 2 * C, 3 * C)):
        words[at] = fmt.trig(k, 20 + k, k & 1)
    _, t, _ = fmt.check(words)
    for k in range(5):
        assert [(6 << 6) | k, k & 1, 20 + k] in t.tolist()


@pytest.mark.parametrize("slab", [1000, "C"])
def test_slabs_equal_the_whole_stream(fmt, C, slab):
    slab = C if slab == "C" else slab
    words = fmt.random(np.random.default_rng(9), 4 * C + 123)
    whole_e, whole_t, whole_s, _ = fmt.decode(words)
    want_e, want_t, want_s = fmt.want(words)
    carry, es, ts, state = None, [], [], None
    for lo in range(0, len(words), slab):
        e, t, s, carry = fmt.decode(words[lo:lo + slab], carry)
        _, _, state = fmt.want(words[lo:lo + slab], state)
        assert s == state                                  # the carried state equals the restatement's, slab by slab
        es.append(e)
        ts.append(t)
    assert np.array_equal(np.concatenate(es), whole_e) and np.array_equal(np.concatenate(ts), whole_t) and s == whole_s
    assert np.array_equal(whole_e, want_e) and np.array_equal(whole_t, want_t) and whole_s == want_s


def test_nothing_past_the_totals_is_touched_and_a_short_capacity_is_refused(fmt, C):
    from event_based_bos_amd import recordings

    words = fmt.random(np.random.default_rng(10), 3 * C + 11)
    want_e, want_t, _ = fmt.want(words)
    w = torch.from_numpy(words.view(np.int64 if fmt.wide else np.int32)).cuda()
    scratch, totals, _ = recordings.evt2_scan(w)
    n_ev, n_tr = totals.tolist()
    assert (n_ev, n_tr) == (len(want_e), len(want_t)) and n_tr > 0
    dtypes = (torch.int16, torch.int16, torch.int64, torch.uint8, torch.int64, torch.uint8, torch.uint8)

    def buffers(n_e, n_t):
        return [torch.full(((n_e if i < 4 else n_t) * torch.empty(0, dtype=d).element_size(),), 0xFF, dtype=torch.uint8, device="cuda").view(d)
                for i, d in enumerate(dtypes)]               # every byte 0xFF

    def untouched(b):
        return bool((b.view(torch.uint8) == 0xFF).all())

    short = buffers(n_ev - 1, n_tr)
    with pytest.raises(RuntimeError, match="event capacity"):
        recordings.evt2_emit(w, scratch, n_ev, n_tr, *short)
    short_t = buffers(n_ev, n_tr - 1)
    with pytest.raises(RuntimeError, match="trigger capacity"):
        recordings.evt2_emit(w, scratch, n_ev, n_tr, *short_t)
    torch.cuda.synchronize()
    assert all(untouched(b) for b in short + short_t)      # refused before any write
    big = buffers(n_ev + 1000, n_tr + 50)
    recordings.evt2_emit(w, scratch, n_ev, n_tr, *big)
    for i, b in enumerate(big):
        assert untouched(b[n_ev if i < 4 else n_tr:])
    got_e = torch.stack([b[:n_ev].to(torch.int64) for b in big[:4]], 1).cpu().numpy()
    got_t = torch.stack([b[:n_tr].to(torch.int64) for b in big[4:]], 1).cpu().numpy()
    assert np.array_equal(got_e, want_e) and np.array_equal(got_t, want_t)


def test_two_runs_give_identical_bytes(fmt, C):
    words = fmt.random(np.random.default_rng(11), 4 * C + 3)
    a, b = fmt.slab(words), fmt.slab(words)
    for u, v in zip(a, b):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    # a device tensor of words at an address that is no multiple of 16 bytes takes the element-wise loads
    signed = np.int64 if fmt.wide else np.int32
    dev = torch.from_numpy(np.concatenate((words[:1], words)).view(signed)).cuda()[1:]
    assert dev.data_ptr() % 16 != 0
    c = fmt.slab(dev)
    for u, v in zip(a, c):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


@pytest.mark.parametrize("chunks", [70, 1093])
def test_scan_pass_beyond_one_wave_and_one_tile(fmt, C, chunks):
    """The scan pass gives wave w the tiles [w per, (w + 1) per) of 64 chunks, per = ceil(tiles / 16): a second wave has work from 65
    chunks, a wave walks a second tile from 1025.  The oracle is the encoder's input (the encoders are held to the restatement on
    the CPU)."""
    from event_based_bos_amd import recordings

    rng = np.random.default_rng(chunks)
    n = chunks * C
    t = np.sort(rng.integers(0, 40_000_001, size=n))
    t[0], t[-1] = 0, 40_000_000
    x, y, p = rng.integers(0, 2048, size=n), rng.integers(0, 2048, size=n), rng.integers(0, 2, size=n)
    triggers = np.stack([np.sort(rng.integers(0, 40_000_001, size=300)), rng.integers(0, 16, size=300), rng.integers(0, 2, size=300)], 1)
    words = recordings.encode_evt21(x, y, t, p, triggers, vectorize=False) if fmt.wide else recordings.encode_evt2(x, y, t, p, triggers)
    n_chunks = -(-len(words) // C)
    assert n_chunks > (64 if chunks == 70 else 1088) and n_chunks % 64 != 0
    s = fmt.slab(words)
    for got, want in zip((s.x, s.y, s.t, s.p, s.trigger_t, s.trigger_id, s.trigger_value), (x, y, t, p, *triggers.T)):
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    last = max(int(t[-1]), int(triggers[-1, 0]))
    assert recordings.carry_to_dict(s.carry) == dict(has_th=1, th=(last >> 6) & TOP, loops=last >> 34)


# ---------------------------------------------------------------------------------------------------- EVT 2.1 only
WIDE = FORMATS[1]


@pytest.mark.parametrize("f", [WIDE], ids=["walk"])
def test_evt21_valid_masks(f):
    masks = [(0, 5), (1, 5), (1 << 31, 5), (0xFFFFFFFF, 2016), (0x80000001, 2047), (0xFFFFFFFF, 2047), (0x00010000, 0)]
    words = [f.th(3)] + [f.ev(k & 1, k, bx, 700 + k, valid) for k, (valid, bx) in enumerate(masks)]
    e, _, _ = f.check(words)
    assert len(e) == 0 + 1 + 1 + 32 + 2 + 32 + 1
    assert e[:, 0].max() == 2047 + 31 and [5 + 31, 702, (3 << 6) | 2, 0] in e.tolist() and [2016 + 31, 703, (3 << 6) | 3, 1] in e.tolist()


@pytest.mark.parametrize("f", [WIDE], ids=["walk"])
def test_evt21_a_chunk_of_all_ones_then_a_sparse_chunk(f):
    from event_based_bos_amd import recordings

    C = recordings.chunk_words("EVT21")
    rng = np.random.default_rng(12)
    dense = f.words([f.ev(k & 1, k & 63, 32 * (k % 40), k % 720, 0xFFFFFFFF) for k in range(C)])
    sparse = f.words([f.ev(k & 1, k & 63, 32 * (k % 40), k % 720, 1 << int(b)) if b >= 0 else f.ev(0, 0, 0, 0, 0)
                      for k, b in enumerate(rng.integers(-8, 32, size=C))])
    words = np.concatenate((f.words([f.th(1)]), dense[:-1], sparse, dense[:37]))
    e, _, _ = f.check(words)
    assert len(e) > 32 * (C - 1)          # the stage runs many rounds in chunk 0


@pytest.mark.parametrize("f", [WIDE], ids=["walk"])
def test_evt21_half_swapped_equals_the_stream_swapped_on_the_host(f):
    from event_based_bos_amd import recordings

    C = recordings.chunk_words("EVT21")
    words = f.random(np.random.default_rng(13), 2 * C + 77)
    swapped = (words << np.uint64(32)) | (words >> np.uint64(32))
    want_e, want_t, want_s = f.want(words)
    assert np.array_equal(ref.decode_evt21(swapped, half_swapped=True)[0], want_e)
    got_e, got_t, got_s, _ = f.decode(swapped, half_swapped=True)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_t, want_t) and got_s == want_s
    plain_e, _, _, _ = f.decode(swapped)                   # and without the flag the swapped stream is another stream
    assert plain_e.shape != want_e.shape or not np.array_equal(plain_e, want_e)


# ---------------------------------------------------------------------------------------------------- DAT
def dat_columns(records, version):
    from event_based_bos_amd import recordings

    cols = recordings.decode_dat(records, version)
    assert tuple(c.dtype for c in cols) == (torch.int16, torch.int16, torch.int64, torch.uint8)
    return torch.stack([c.to(torch.int64) for c in cols], 1).cpu().numpy()


@pytest.mark.parametrize("version", [1, 2])
def test_dat_decode(version):
    records, events = ((ref.DAT1_EXAMPLE_RECORDS, ref.DAT1_EXAMPLE_EVENTS) if version == 1 else (ref.DAT2_EXAMPLE_RECORDS, ref.DAT2_EXAMPLE_EVENTS))
    assert dat_columns(np.array(records, dtype=np.uint32), version).tolist() == [list(v) for v in events]
    rng = np.random.default_rng(15)
    for n in (0, 1, 2, 255, 256, 513, 70001):               # odd and even counts, more than one workgroup
        records = rng.integers(0, 1 << 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(dat_columns(records, version), ref.decode_dat(records, version))


def test_dat_fourteen_bit_addresses_and_the_capacity_guard():
    from event_based_bos_amd import _hip, recordings

    records = recordings.encode_dat([16383, 0, 16383, 8192], [0, 16383, 16383, 8191], [0, 1, (1 << 32) - 1, (1 << 32) - 1], [1, 0, 1, 0])
    assert dat_columns(records, 2).tolist() == [[16383, 0, 0, 1], [0, 16383, 1, 0], [16383, 16383, (1 << 32) - 1, 1], [8192, 8191, (1 << 32) - 1, 0]]
    # straight through the entry: columns one element longer than the records stay 0xFF there, at odd and even counts and with
    # columns that do not allow the paired stores; a capacity below the count is refused before any write
    lib = _hip.require_gpu()
    rng = np.random.default_rng(16)
    for n, shift in ((1001, 0), (1000, 0), (1001, 1), (1000, 1)):
        rec = rng.integers(0, 1 << 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
        r = torch.from_numpy(rec.reshape(-1).view(np.int32)).cuda()
        cols = [torch.full((n + 2,), -1, dtype=d, device="cuda")[shift:shift + n + 1] for d in (torch.int16, torch.int16, torch.int64, torch.int8)]
        assert lib.ebos_dat_decode(_hip.ptr(r), n, 2, *(_hip.ptr(c) for c in cols), n - 1, _hip.stream_ptr(r.device)) == -1
        torch.cuda.synchronize()
        assert all(bool((c == -1).all()) for c in cols)
        _hip.check(lib.ebos_dat_decode(_hip.ptr(r), n, 2, *(_hip.ptr(c) for c in cols), n + 1, _hip.stream_ptr(r.device)), "ebos_dat_decode")
        got = torch.stack([c[:n].to(torch.int64) & m for c, m in zip(cols, (0xFFFF, 0xFFFF, -1, 0xFF))], 1).cpu().numpy()
        assert np.array_equal(got, ref.decode_dat(rec, 2)) and all(int(c[n]) == -1 for c in cols)


# ---------------------------------------------------------------------------------------------------- files
@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """A synthetic recording, the same events and trigger edges as an EVT 3.0 file, and that file's store."""
    from event_based_bos_amd import RawEventStore, evt3
    from event_based_bos_amd.data_loader import _trigger_rows
    from event_based_bos_amd.evaluation import synthetic_recording

    d = str(tmp_path_factory.mktemp("recordings"))
    shape = (64, 96)
    ev_path, fr_path, tr_path, stamps = synthetic_recording(d, shape, 6, 3000)
    c = RawEventStore(ev_path).event_data
    rows, layout = _trigger_rows(tr_path)
    assert layout == "old"
    raw3 = os.path.join(d, "evt3.raw")
    evt3.write_raw_file(raw3, evt3.encode_evt3(c["x"], c["y"], c["t"], c["p"], rows), shape[1], shape[0])
    return dict(dir=d, cols=c, rows=rows, shape=shape, store3=RawEventStore(raw3))


def same_columns(store, other):
    assert len(store) == len(other) > 10_000 and store.dropped_outside == other.dropped_outside == 0
    for k in "xytp":
        assert store.event_data[k].dtype == other.event_data[k].dtype and np.array_equal(store.event_data[k], other.event_data[k]), k


@pytest.mark.parametrize("name", ["EVT2", "EVT21", "EVT21-legacy"])
def test_raw_files_of_every_format_through_the_event_store(recording, name):
    from event_based_bos_amd import RawEventStore, recordings

    r, c = recording, recording["cols"]
    path = os.path.join(r["dir"], name + ".raw")
    H, W = r["shape"]
    if name == "EVT2":
        recordings.write_raw_file(path, recordings.encode_evt2(c["x"], c["y"], c["t"], c["p"], r["rows"]), W, H, "EVT2")
    else:
        words = recordings.encode_evt21(c["x"], c["y"], c["t"], c["p"], r["rows"])
        if name == "EVT21":
            recordings.write_raw_file(path, words, W, H, "EVT21")
        else:                                            # a legacy file: `% evt 2.1` alone, the halves exchanged
            with open(path, "wb") as f:
                f.write(f"% evt 2.1\n% geometry {W}x{H}\n% end\n".encode("ascii") + ((words << np.uint64(32)) | (words >> np.uint64(32))).astype("<u8").tobytes())
    store = RawEventStore(path)
    assert store.header.format == name.split("-")[0] and (store.header.height, store.header.width) == r["shape"]
    same_columns(store, r["store3"])
    assert store.triggers.dtype == np.int64 and np.array_equal(store.triggers, r["store3"].triggers) and len(store.triggers) > 0
    # slabs that cut the file anywhere, and a tail that is no whole word, give the same columns
    odd = os.path.join(r["dir"], name + "_odd.raw")
    with open(path, "rb") as f, open(odd, "wb") as g:
        g.write(f.read() + b"\x20\x21\x22")
    x, y, t, p, triggers, _ = recordings.decode_recording(odd, slab_words=4099)
    assert np.array_equal(x, store.event_data["x"]) and np.array_equal(t, store.event_data["t"]) and np.array_equal(triggers, r["rows"])
    if name == "EVT21-legacy":                           # the override reads the same bytes as plain words: another stream
        other = RawEventStore(path, half_swapped=False)
        assert len(other) != len(store) or not np.array_equal(other.event_data["x"], store.event_data["x"])


@pytest.mark.parametrize("header", [True, False], ids=["header", "bare"])
def test_dat_file_through_the_event_store(recording, header):
    from event_based_bos_amd import RawEventStore, recordings

    r, c = recording, recording["cols"]
    H, W = r["shape"]
    path = os.path.join(r["dir"], f"rec_{int(header)}_td.dat")
    recordings.write_dat_file(path, recordings.encode_dat(c["x"], c["y"], c["t"], c["p"]), W, H, header=header)
    if not header:
        with pytest.raises(ValueError, match="geometry"):
            RawEventStore(path)
    store = RawEventStore(path, sensor_size=None if header else (H, W))
    assert store.header.format == "DAT" and (store.header.height, store.header.width) == r["shape"]
    same_columns(store, r["store3"])
    assert store.triggers.shape == (0, 3) and store.triggers.dtype == np.int64
    x, y, t, p, _, _ = recordings.decode_recording(path, slab_words=4099, sensor_size=(H, W))
    assert np.array_equal(x, store.event_data["x"]) and np.array_equal(t, store.event_data["t"])


def test_events_outside_the_geometry_are_dropped(recording):
    from event_based_bos_amd import RawEventStore, recordings

    r, c = recording, recording["cols"]
    H, W = r["shape"]
    path = os.path.join(r["dir"], "narrow.raw")
    recordings.write_raw_file(path, recordings.encode_evt2(c["x"], c["y"], c["t"], c["p"]), W, H, "EVT2")
    store = RawEventStore(path, sensor_size=(H - 10, W - 7))
    keep = (c["x"] < W - 7) & (c["y"] < H - 10)
    assert store.dropped_outside == int((~keep).sum()) > 0 and len(store) == int(keep.sum())
    for k in "xytp":
        assert np.array_equal(store.event_data[k], c[k][keep]), k
