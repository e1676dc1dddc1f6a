"""The EVT 3.0 decode on the GPU (csrc/evt3.hip) against the sequential restatement of the word rules (tests/_evt3_ref.py): every
comparison is exact equality of integer arrays -- events, triggers and the carried state -- with the streams aimed at the seams
between the chunks of C = ebos_evt3_chunk_words() words."""
import os

import numpy as np
import pytest
import torch

import _evt3_ref as ref

pytestmark = pytest.mark.gpu

TH, TL, AY, AX, VB, V12, V8, TRIG = (k << 12 for k in (ref.TIME_HIGH, ref.TIME_LOW, ref.ADDR_Y, ref.ADDR_X, ref.VECT_BASE_X, ref.VECT_12,
                                                       ref.VECT_8, ref.EXT_TRIGGER))


@pytest.fixture(scope="module")
def C():
    from event_based_bos_amd import evt3

    return evt3.chunk_words()


def gpu_decode(words, carry=None):
    """(events [n, 4], triggers [m, 3], state dict, the device carry) in the restatement's layout."""
    from event_based_bos_amd import evt3

    s = evt3.decode_evt3(np.asarray(words, dtype=np.uint16), carry)
    assert (s.x.dtype, s.y.dtype, s.t.dtype, s.p.dtype) == (torch.int16, torch.int16, torch.int64, torch.uint8)
    assert (s.trigger_t.dtype, s.trigger_value.dtype, s.trigger_id.dtype) == (torch.int64, torch.uint8, torch.uint8)
    events = torch.stack([c.to(torch.int64) for c in (s.x, s.y, s.t, s.p)], 1).cpu().numpy()
    triggers = torch.stack([c.to(torch.int64) for c in (s.trigger_t, s.trigger_value, s.trigger_id)], 1).cpu().numpy()
    return events, triggers, evt3.carry_to_dict(s.carry), s.carry


def check(words, state=None):
    from event_based_bos_amd import evt3

    want_e, want_t, want_s = ref.decode(words, state)
    got_e, got_t, got_s, _ = gpu_decode(words, None if state is None else evt3.new_carry("cuda", state))
    assert got_e.shape == want_e.shape and np.array_equal(got_e, want_e)
    assert got_t.shape == want_t.shape and np.array_equal(got_t, want_t)
    assert got_s == want_s
    return want_e, want_t, want_s


def filler(rng, n):
    """Words without a TIME_HIGH: addresses, vectors, triggers, time lows and ignored types."""
    return ref.random_words(rng, n, p_time_high=0.0)


def test_worked_example():
    e, t, s = check(ref.EXAMPLE_WORDS)
    assert e.tolist() == [list(v) for v in ref.EXAMPLE_EVENTS] and t.tolist() == [list(v) for v in ref.EXAMPLE_TRIGGERS]


def test_random_stream_over_every_word_type(C):
    words = ref.random_words(np.random.default_rng(1), 10 * C + 37)
    assert set((words >> 12).tolist()) == set(range(16))
    e, t, s = check(words)
    assert len(e) > C and len(t) > 10 and s["loops"] > 0
    check(words[5:], dict(has_th=1, th=4090, tl=77, y=301, bx=65530, pol=1, loops=(1 << 33) + 2))   # from a carried state, t past 2^57


def test_vector_base_and_vector_word_across_a_seam(C):
    rng = np.random.default_rng(2)
    words = np.concatenate(([TH | 5, AY | 9], filler(rng, 2 * C - 2), filler(rng, 100)))
    words[C - 1], words[C] = VB | 0x800 | 700, V12 | 0xA5A
    e, _, _ = check(words)
    at = (e[:, 0] == 701) & (e[:, 3] == 1)
    assert at.any()      # bit 1 of the mask on the base of the chunk before


def test_wrap_at_a_seam_resets_time_low(C):
    rng = np.random.default_rng(3)
    words = np.concatenate(([TH | 4000], filler(rng, 3 * C)))
    words[C - 2], words[C - 1], words[C], words[C + 1] = TL | 0x123, TH | 4095, TH | 0, AX | 17
    e, _, s = check(words)
    assert s["loops"] == 1 and [17, 1 << 24] in e[:, [0, 2]].tolist()   # tl = 0 after the wrap, not 0x123


def test_chunks_without_time_high_and_of_state_words_only(C):
    rng = np.random.default_rng(4)
    state_only = np.where(rng.random(C) < 0.5, TL, AY) | rng.integers(0, 2048, size=C)
    words = np.concatenate(([TH | 1], filler(rng, C - 1), filler(rng, C), state_only, [VB | 3], state_only[:50], filler(rng, C // 2)))
    assert not np.any((words[C:3 * C] >> 12) == ref.TIME_HIGH)
    check(words)
    check(np.concatenate(([TH | 1], state_only, state_only)))          # no event at all


def test_first_time_high_in_the_third_chunk(C):
    rng = np.random.default_rng(5)
    words = np.concatenate((filler(rng, 2 * C + 100), [TH | 77], filler(rng, C)))
    words[10], words[2 * C + 99] = AY | 555, AX | 1               # an ADDR_Y before the first TIME_HIGH does not count
    words[2 * C + 101] = AX | 2
    e, _, _ = check(words)
    assert e[0].tolist() == [2, 0, 77 << 12, 0]


def test_no_time_high_at_all_gives_nothing(C):
    words = filler(np.random.default_rng(6), 3 * C + 5)
    e, t, s = check(words)
    assert len(e) == 0 and len(t) == 0 and s == ref.START


def test_lengths_around_a_chunk(C):
    rng = np.random.default_rng(7)
    stream = ref.random_words(rng, C + 1, p_time_high=0.05)
    stream[0] = TH | 9
    for n in (0, 1, C - 1, C, C + 1):
        check(stream[:n])
        check(stream[1:1 + n][:n], dict(has_th=1, th=3, tl=4, y=5, bx=6, pol=1, loops=7))


def test_twelve_events_a_word(C):
    words = np.concatenate(([TH | 1, AY | 3, VB | 0x800 | 0], np.full(3 * C, V12 | 0xFFF)))
    e, _, s = check(words)
    assert len(e) == 12 * 3 * C and s["bx"] == (12 * 3 * C) & 0xFFFF


@pytest.mark.parametrize("slab", [1000, "C"])
def test_slabs_equal_the_whole_stream(C, slab):
    slab = C if slab == "C" else slab
    words = ref.random_words(np.random.default_rng(8), 6 * C + 123)
    whole_e, whole_t, whole_s, _ = gpu_decode(words)
    carry, es, ts = None, [], []
    for lo in range(0, len(words), slab):
        e, t, s, carry = gpu_decode(words[lo:lo + slab], carry)
        es.append(e)
        ts.append(t)
    assert np.array_equal(np.concatenate(es), whole_e) and np.array_equal(np.concatenate(ts), whole_t) and s == whole_s
    want_e, want_t, want_s = ref.decode(words)
    assert np.array_equal(whole_e, want_e) and np.array_equal(whole_t, want_t) and whole_s == want_s


def test_nothing_past_the_totals_is_touched_and_a_short_capacity_is_refused(C):
    from event_based_bos_amd import evt3

    words = ref.random_words(np.random.default_rng(9), 3 * C + 11)
    want_e, want_t, _ = ref.decode(words)
    w = torch.from_numpy(words.view(np.int16)).cuda()
    scratch, totals, _ = evt3.evt3_scan(w)
    n_ev, n_tr = totals.tolist()
    assert (n_ev, n_tr) == (len(want_e), len(want_t)) and n_tr > 0
    dtypes = (torch.int16, torch.int16, torch.int64, torch.uint8, torch.int64, torch.uint8, torch.uint8)

    def buffers(n_e, n_t):
        return [torch.full((n_e if i < 4 else n_t,), 0x5A, dtype=d, device="cuda") for i, d in enumerate(dtypes)]

    short = buffers(n_ev - 1, n_tr)
    with pytest.raises(RuntimeError, match="event capacity"):
        evt3.evt3_emit(w, scratch, n_ev, n_tr, *short)
    short_t = buffers(n_ev, n_tr - 1)
    with pytest.raises(RuntimeError, match="trigger capacity"):
        evt3.evt3_emit(w, scratch, n_ev, n_tr, *short_t)
    torch.cuda.synchronize()
    assert all(bool((b == 0x5A).all()) for b in short + short_t)      # refused before any write
    big = buffers(n_ev + 1000, n_tr + 50)
    evt3.evt3_emit(w, scratch, n_ev, n_tr, *big)
    for i, b in enumerate(big):
        n = n_ev if i < 4 else n_tr
        assert bool((b[n:] == 0x5A).all())
    got_e = torch.stack([b[:n_ev].to(torch.int64) for b in big[:4]], 1).cpu().numpy()
    got_t = torch.stack([b[:n_tr].to(torch.int64) for b in big[4:]], 1).cpu().numpy()
    assert np.array_equal(got_e, want_e) and np.array_equal(got_t, want_t)


def test_two_runs_give_identical_bytes(C):
    from event_based_bos_amd import evt3

    words = ref.random_words(np.random.default_rng(10), 5 * C + 3)
    a, b = evt3.decode_evt3(words), evt3.decode_evt3(words)
    for u, v in zip(a, b):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    # a device tensor of words at an address that is no multiple of 16 bytes takes the element-wise loads
    dev = torch.from_numpy(np.concatenate(([0], words)).astype(np.uint16).view(np.int16)).cuda()[1:]
    c = evt3.decode_evt3(dev)
    for u, v in zip(a, c):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def raw_recording(tmp_path_factory):
    """A synthetic recording and the same events and trigger edges as a .raw file written by the package's encoder."""
    from event_based_bos_amd import RawEventStore, evt3
    from event_based_bos_amd.data_loader import _trigger_rows
    from event_based_bos_amd.evaluation import synthetic_recording

    d = str(tmp_path_factory.mktemp("evt3_recording"))
    shape = (64, 96)
    ev_path, fr_path, tr_path, stamps = synthetic_recording(d, shape, 6, 3000)
    cols = RawEventStore(ev_path)
    rows, layout = _trigger_rows(tr_path)
    assert layout == "old"
    c = cols.event_data
    words = evt3.encode_evt3(c["x"], c["y"], c["t"], c["p"], rows)
    raw = os.path.join(d, "cd_events.raw")
    evt3.write_raw_file(raw, words, shape[1], shape[0])
    return dict(raw=raw, cols=cols, frames=fr_path, triggers=tr_path, rows=rows, shape=shape, words=words)


def test_raw_file_through_the_event_store(raw_recording, tmp_path):
    from event_based_bos_amd import FrameStore, RawEventStore

    r = raw_recording
    store = RawEventStore(r["raw"])
    assert store.header.format == "EVT3" and (store.header.height, store.header.width) == r["shape"] and store.dropped_outside == 0
    assert len(store) == len(r["cols"]) > 10_000
    for k in "xytp":
        assert store.event_data[k].dtype == r["cols"].event_data[k].dtype and np.array_equal(store.event_data[k], r["cols"].event_data[k]), k
    assert np.array_equal(store.load_event(100, 5000), r["cols"].load_event(100, 5000))
    assert store.triggers.dtype == np.int64 and np.array_equal(store.triggers, r["rows"])
    a, b = FrameStore(r["frames"], store.triggers), FrameStore(r["frames"], r["triggers"])
    assert len(a.timestamps) == 6 and np.array_equal(a.timestamps, b.timestamps)
    # slabs that cut the file anywhere, and an odd trailing byte, give the same columns
    from event_based_bos_amd import evt3

    odd = str(tmp_path / "odd.raw")
    with open(r["raw"], "rb") as f, open(odd, "wb") as g:
        g.write(f.read() + b"\x20")
    x, y, t, p, triggers, _ = evt3.decode_raw_file(odd, slab_words=4099)
    assert np.array_equal(x, store.event_data["x"]) and np.array_equal(t, store.event_data["t"]) and np.array_equal(triggers, r["rows"])


def test_events_outside_the_geometry_are_dropped(raw_recording, tmp_path):
    from event_based_bos_amd import RawEventStore, evt3

    r = raw_recording
    H, W = r["shape"]
    path = str(tmp_path / "narrow.raw")
    with open(path, "wb") as f:                       # no geometry in the header: the caller's sensor_size decides
        f.write(b"% evt 3.0\n% end\n" + r["words"].astype("<u2").tobytes())
    with pytest.raises(ValueError, match="geometry"):
        RawEventStore(path)
    store = RawEventStore(path, sensor_size=(H - 10, W - 7))
    c = r["cols"].event_data
    keep = (c["x"] < W - 7) & (c["y"] < H - 10)
    assert store.dropped_outside == int((~keep).sum()) > 0 and len(store) == int(keep.sum())
    for k in "xytp":
        assert np.array_equal(store.event_data[k], c[k][keep]), k
    # t past 2^31 us stays int64
    late = str(tmp_path / "late.raw")
    t = c["t"][:2000].astype(np.int64) + (1 << 31)
    evt3.write_raw_file(late, evt3.encode_evt3(c["x"][:2000], c["y"][:2000], t, c["p"][:2000]), W, H)
    store = RawEventStore(late)
    assert store.event_data["t"].dtype == np.int64 and np.array_equal(store.event_data["t"], t)


@pytest.mark.parametrize("chunks", [70, 1093])
def test_scan_pass_beyond_one_wave_and_one_tile(C, chunks):
    """The scan pass gives wave w the tiles [w per, (w + 1) per) of 64 chunks, per = ceil(tiles / 16): a second wave has work from 65
    chunks, a wave walks a second tile from 1025.  The oracle is the encoder's input (the encoder is held to the restatement on the
    CPU), over two wraps of the 24-bit time so that the loop count crosses the waves."""
    from event_based_bos_amd import evt3

    rng = np.random.default_rng(chunks)
    n = chunks * C
    t = np.sort(rng.integers(0, 40_000_001, size=n))
    t[0], t[-1] = 0, 40_000_000
    x, y, p = rng.integers(0, 2048, size=n), rng.integers(0, 2048, size=n), rng.integers(0, 2, size=n)
    triggers = np.stack([np.sort(rng.integers(0, 40_000_001, size=300)), rng.integers(0, 16, size=300), rng.integers(0, 2, size=300)], 1)
    words = evt3.encode_evt3(x, y, t, p, triggers, vectorize=False)
    n_chunks = -(-len(words) // C)
    assert n_chunks > (64 if chunks == 70 else 1088) and n_chunks % 64 != 0
    s = evt3.decode_evt3(words)
    for got, want in zip((s.x, s.y, s.t, s.p, s.trigger_t, s.trigger_id, s.trigger_value), (x, y, t, p, *triggers.T)):
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    last = max(int(t[-1]), int(triggers[-1, 0]))
    state = evt3.carry_to_dict(s.carry)
    assert (state["has_th"], state["loops"], state["th"]) == (1, last >> 24, (last >> 12) & 0xFFF) and state["loops"] == 2
