"""tests/_splat_ordered_ref.py -- the numpy restatement of the ordered vote's index and summation order -- pinned without a GPU against
the float64 oracle, on the cases of tests/_ops_cases.py.  tests/test_gpu_splat_ordered.py then holds the kernels to the restatement bit
for bit."""
import numpy as np
import pytest

import _ops_cases as C
import _splat_ordered_ref as R

IDS = dict(ids=lambda c: c.id)
CASES = C.SMALL_EVENT_CASES + tuple(C.EventCase(1, C.N_BIG, dt, pad) for dt, pad in ((np.float32, 2), (np.float64, 0)))


def weighted_bar(case, err_cpu_f32):
    """The rule of tests/test_gpu_ops.py (``splat_all_modes``): the project's image bar; in float32 raised to 10 x the error of the same
    float32 sum in input order on the CPU, never above 1e-4."""
    bar = C.bar(case.dtype, "image")
    return bar if case.dtype == np.float64 else min(max(bar, 10.0 * err_cpu_f32), 1e-4)


def within(err, case, bar):
    return err <= bar if case.dtype == np.float64 else err < bar


def test_threshold_is_read_from_the_source():
    assert 64 <= R.long_list_threshold() <= 4096


@pytest.mark.parametrize("case", CASES, **IDS)
def test_unit_weight_equals_the_oracle_exactly(case):
    """On the 1/64 px grid every tap is a multiple of 1 / 4096 and every sum exact: any order gives the oracle's image."""
    ev, pad, size = C.splat_events(case), case.pad, C.padded(case.pad)
    np.testing.assert_array_equal(R.vote(ev, size, (pad, pad), weight=1.0), C.ref_splat(ev, pad).astype(case.dtype))
    np.testing.assert_array_equal(R.vote(ev, size, (pad, pad), mode=R.COUNT), C.ref_count(ev, pad).astype(case.dtype))
    if case.n:
        np.testing.assert_array_equal(R.vote(ev, size, (pad, pad), mode=R.POLARITY), C.ref_polarity(ev, pad).astype(case.dtype))
    else:
        assert not R.vote(ev, size, (pad, pad), mode=R.POLARITY).any()


@pytest.mark.parametrize("case", CASES, **IDS)
def test_weighted_votes_within_the_bars(case):
    ev, wt, pad, size = C.splat_events(case), C.weights_of(case), case.pad, C.padded(case.pad)
    if case.n == 0:
        assert not R.vote(ev, size, (pad, pad), weight=wt).any()
        return
    f32 = case.dtype == np.float32
    pos = ev[..., 3] > 0
    for tag, weight in (("per-event", wt), ("scalar", 0.7)):
        w32 = wt if tag == "per-event" else np.full(wt.shape, 0.7, dtype=np.float32)
        want = C.ref_splat(ev, pad, weight)
        cpu = C.rel(C.ref_splat_f32_in_order(ev, pad, w32), want) if f32 else 0.0
        err, bar = C.rel(R.vote(ev, size, (pad, pad), weight=weight), want), weighted_bar(case, cpu)
        print(f"{case.id} bilinear {tag}: {err:.3e} (float32 in input order {cpu:.3e}, bar {bar:.3e})")
        assert within(err, case, bar), (tag, err, bar)
        want = C.ref_polarity(ev, pad, weight)
        cpu = C.rel(np.stack([C.ref_splat_f32_in_order(ev, pad, w32 * m) for m in (pos, ~pos)], axis=1), want) if f32 else 0.0
        err, bar = C.rel(R.vote(ev, size, (pad, pad), weight=weight, mode=R.POLARITY), want), weighted_bar(case, cpu)
        print(f"{case.id} polarity {tag}: {err:.3e} (float32 in input order {cpu:.3e}, bar {bar:.3e})")
        assert within(err, case, bar), (tag, err, bar)


def test_long_lists_take_the_wave_order():
    """Exactly the threshold: one running sum in list order.  One addend more: 64 lane-strided partial sums and the fixed reduction --
    both written out here as scalar loops."""
    thr = R.long_list_threshold()
    for n in (thr, thr + 1):
        rs = np.random.RandomState(3)
        ev = np.zeros((1, n, 4), dtype=np.float32)
        ev[0, :, 0], ev[0, :, 1] = 17.25, 23.5
        wt = rs.uniform(0.5, 1.5, (1, n)).astype(np.float32)
        got = R.vote(ev, C.EVENT_IMAGE, weight=wt)
        addends = (np.float32(0.75) * np.float32(0.5)) * wt[0]
        if n <= thr:
            want = np.float32(0)
            for v in addends:
                want = want + v
        else:
            p = [np.float32(0)] * 64
            for j, v in enumerate(addends):
                p[j % 64] = p[j % 64] + v
            for off in (32, 16, 8, 4, 2, 1):
                for lane in range(off):
                    p[lane] = p[lane] + p[lane + off]
            want = p[0]
        assert got[0, 17, 23] == want and got.dtype == np.float32
        assert C.rel(got, C.ref_splat(ev, 0, wt)) < 1e-5
        assert np.count_nonzero(got) == 4


def test_refusals_come_before_any_launch():
    """Sizes the ordered route refuses, a short workspace, unknown routes: all before any HIP call, so without a GPU."""
    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    lib = ebos._hip.load_library()
    h, w = C.EVENT_IMAGE
    refused = lambda rc, text: rc == -1 and text in lib.ebos_last_error()
    need = int(lib.ebos_splat_index_bytes(3, 257, h, w, 0))
    assert need >= 4 * (3 * (h + 1) * (w + 1) + 1) + 4 * 3 * 257
    assert refused(lib.ebos_splat_index_build_f32(0x1000, 0, 1e-6, 3, 257, h, w, 0, 0, 0x1000, need - 1, None), b"too small")
    assert refused(lib.ebos_splat_ordered_f64(0x1000, None, 1.0, 0, 1e-6, 3, 257, h, w, 0, 0, 0x1000, need - 1, 0x1000, None), b"too small")
    for b, n, hh, ww, text in ((65536, 10, h, w, b"bad sizes"), (1, 2 ** 31, h, w, b"2^31"), (65535, 32769, h, w, b"2^31"),
                               (1, 10, 46341, 46341, b"2^31")):
        assert int(lib.ebos_splat_index_bytes(b, n, hh, ww, 0)) == 0
        assert refused(lib.ebos_splat_index_build_f64(None, 0, 1e-6, b, n, hh, ww, 0, 0, None, 0, None), text)
        assert refused(lib.ebos_splat_ordered_f32(None, None, 1.0, 0, 1e-6, b, n, hh, ww, 0, 0, None, 0, None, None), text)
    with pytest.raises(ValueError):
        ebos.ops.splat(torch.zeros(1, 3, 4), (h, w), route="sorted")
    with pytest.raises(ValueError):
        ebos.EventImageConverter((h, w), vote="sorted")
    assert ebos.EventImageConverter((h, w)).vote == "atomic"


@pytest.mark.parametrize("polarity", (False, True))
@pytest.mark.parametrize("case", (C.EventCase(3, 257, np.float32, 2), C.EventCase(3, 257, np.float64, 0), C.EventCase(1, C.N_BIG, np.float32, 0)),
                         **IDS)
def test_index_groups_by_key_in_ascending_order(case, polarity):
    ev = C.splat_events(case).copy()
    n = case.n
    planted = {5: np.nan, 6: np.inf, 7: -np.inf, 9: 2.0 ** 30, 10: -2.0 ** 31, 12: 3e38}
    for e, v in planted.items():
        ev[:, e, e % 2] = v
    pad, (h, w) = case.pad, C.padded(case.pad)
    offsets, indices = R.build_index(ev, (h, w), (pad, pad), polarity=polarity)
    planes = 2 if polarity else 1
    n_keys = case.b * planes * (h + 1) * (w + 1)
    assert offsets.shape == (n_keys + 1,) and indices.shape == (case.b * n,) and offsets[0] == 0
    assert (np.diff(offsets) >= 0).all()
    assert sorted(indices.tolist()) == list(range(case.b * n))            # every event once
    kept, dropped = indices[:offsets[-1]], indices[offsets[-1]:]
    # dropped: exactly the events whose four taps the oracle masks, and the planted ones
    with np.errstate(invalid="ignore"):
        safe = np.where(np.isfinite(ev) & (np.abs(ev) < 2.0 ** 29), ev, -100.0)     # (the oracle takes no NaN: far outside instead)
    all_masked = ~C.tap_masks(safe, pad).any(axis=1)                      # [b, n]
    for e in planted:
        assert all_masked[:, e].all()
    np.testing.assert_array_equal(np.sort(dropped), np.flatnonzero(all_masked.reshape(-1)))
    assert (np.diff(dropped) > 0).all()
    assert 0 < len(dropped) < case.b * n
    # grouped by key, ascending inside a key
    run = np.repeat(np.arange(n_keys), np.diff(offsets))
    same = run[1:] == run[:-1]
    assert (np.diff(kept)[same] > 0).all()
    # the key of every kept event, from the oracle's own top-left tap
    e64 = ev.reshape(-1, 4)[kept].astype(np.float64)
    base = np.floor(e64[:, :2] + 1e-6)         # (coordinates on the 1/64 px grid: the same floor in float32 and float64)
    row = kept // n
    img = row * planes + (np.where(e64[:, 3] > 0, 0, 1) if polarity else 0)
    np.testing.assert_array_equal(run, (img * (h + 1) + base[:, 0].astype(np.int64) + pad + 1) * (w + 1) + base[:, 1].astype(np.int64) + pad + 1)
