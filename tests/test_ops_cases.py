"""tests/_ops_cases.py pinned without a GPU: every (kernel, case) pair the table claims takes at least two trips of the kernel's loop with
the LAUNCH LIMITS AS THE C SOURCES STATE THEM, the last trip ragged; an evaluation that stopped after the first trip misses the case's
bar by a factor of 100 and more (by the oracle alone: a kernel that dropped its later trips could not pass tests/test_gpu_ops.py); the
planted edge events are what the table states; the oracle agrees with itself in its numpy and torch forms."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import _ops_cases as C
from _ops_cases import O

LIM = C.limits()
BIG32 = C.EventCase(3, C.N_BIG, np.float32, 2)
BIG64 = C.EventCase(1, C.N_BIG, np.float64, 0)
FACTOR = 100.0


def check_claims(lim):
    """Every claim reaches a second trip, and its last trip is partial."""
    for claim in C.claims():
        kernel = claim[0]
        if kernel in C.REGION_KERNELS:
            _, case, rows, cols = claim
            for what, items, step in (("rows", rows, lim["kCostGrid"]), ("columns", cols, lim["kCostBlock"])):
                assert -(-items // step) >= 2 and items % step != 0, f"{kernel} on {case}: {items} {what} in steps of {step}"
        else:
            _, case, items = claim
            n_trips, last, wave = C.trips(items, *lim[kernel])
            assert n_trips >= 2 and 0 < last < wave, f"{kernel} on {case}: {items} items, {n_trips} trip(s) of {wave}, last {last}"


def test_limits_are_read_from_the_sources():
    assert set(C.STREAM_KERNELS) | {"default_cap", "kCostGrid", "kCostBlock"} == set(LIM)
    for kernel in C.STREAM_KERNELS:
        block, cap = LIM[kernel]
        assert block > 0 and cap > 0
    # kernels that name no cap run under stream_grid's default; the others under the cap of their call site
    assert LIM["warp_dense_kernel"][1] == LIM["splat_kernel"][1] == LIM["default_cap"]


def test_every_claim_takes_a_second_ragged_trip():
    check_claims(LIM)
    # n_big: two trips under the default cap, three under the cap of time_range / warp_2dof_bwd
    assert C.trips(C.N_BIG, *LIM["splat_kernel"])[0] == 2
    assert C.trips(C.N_BIG, *LIM["time_range_kernel"])[0] == 3 and C.trips(C.N_BIG, *LIM["warp_2dof_bwd_kernel"])[0] == 3
    # the element-wise image is the smallest-but-one-row past the LARGEST cap of its kernels
    largest = max(LIM[k][0] * LIM[k][1] for k in C.PIXEL_KERNELS)
    assert largest < C.PIXEL_IMAGE[0] * C.PIXEL_IMAGE[1] < largest + 20 * C.PIXEL_IMAGE[1]
    # the cost image is the smallest whose cropped region still exceeds the grid and the block
    assert C.COST_IMAGE == (LIM["kCostGrid"] + 3, LIM["kCostBlock"] + 3)


@pytest.mark.parametrize("name,pattern,replacement", [
    ("common.h", r"max_blocks = 256 \* 8", "max_blocks = 256 * 16"),                               # the default cap
    ("warp_kernels.hip", r"stream_grid\(n, 256, 1024\), \(unsigned\)b", "stream_grid(n, 256, 4096), (unsigned)b"),   # time_range
    ("cost_kernels.hip", r"kCostBlock, 4096\), K", "kCostBlock, 8192), K"),                        # gradmag_grad
    ("image_filters.hip", r"inner, 256, 4096", "inner, 256, 1 << 13"),                             # a cap the table cannot read
    ("cost_kernels.hip", r"constexpr int kCostGrid = 240;", "constexpr int kCostGrid = 480;"),
    ("cost_kernels.hip", r"constexpr int kCostBlock = 256;", "constexpr int kCostBlock = 512;"),
])
def test_a_raised_cap_fails_the_claims(tmp_path, name, pattern, replacement):
    """On a scratch copy of the sources: a cap raised past a case (or written so that the table cannot read it) is an error here,
    not a loop the GPU tests quietly stop covering."""
    for f in ("common.h", "warp_kernels.hip", "splat_kernels.hip", "cost_kernels.hip", "image_filters.hip"):
        shutil.copy(os.path.join(C.CSRC, f), tmp_path / f)
    check_claims(C.limits(str(tmp_path)))          # the copy as it is passes
    text = (tmp_path / name).read_text()
    edited, count = re.subn(pattern, replacement, text)
    assert count >= 1, f"{pattern!r} not found in {name}"
    (tmp_path / name).write_text(edited)
    with pytest.raises((AssertionError, C.LimitNotFound)):
        check_claims(C.limits(str(tmp_path)))


def test_a_missing_limit_is_an_error(tmp_path):
    for f in ("common.h", "warp_kernels.hip", "splat_kernels.hip", "cost_kernels.hip", "image_filters.hip"):
        shutil.copy(os.path.join(C.CSRC, f), tmp_path / f)
    (tmp_path / "common.h").write_text((tmp_path / "common.h").read_text().replace("int max_blocks = 256 * 8", "int max_blocks"))
    with pytest.raises(C.LimitNotFound):
        C.limits(str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- planted events
@pytest.mark.parametrize("case", [BIG32, BIG64, C.MIXED_CASES[0]], ids=lambda c: c.id)
def test_planted_events_are_what_the_table_states(case):
    ev = C.splat_events(case)
    assert ev.dtype == case.dtype and ev.shape == (case.b, case.n, 4)
    if case.dtype == np.float32:
        assert np.array_equal(ev[..., :2] * 64, np.rint(ev[..., :2] * 64))      # the 1/64 px grid, exact in float32
    masked = C.counted_masked_taps(ev, case.pad)
    stated = C.stated_masked_taps(case)
    assert stated > 0 and (masked.sum(axis=1) == stated).all()
    idx, rc, cc = C.edge_categories(case.n)
    per_event = masked[:, idx]
    # an axis masks its first tap, its second or both: events with 2, 3 and 4 masked taps, and every tap is somewhere the only valid one
    assert set(np.unique(per_event)) == {2, 3, 4} and (np.delete(masked, idx, axis=1) == 0).all()
    mask = C.tap_masks(ev, case.pad)
    for tap in range(4):
        others = [t for t in range(4) if t != tap]
        assert (mask[:, tap] & ~mask[:, others].any(axis=1)).any(axis=1).all(), f"tap {tap} is never the only valid one"
    assert (ev[..., 3] <= 0).sum(axis=1).tolist() == [C.stated_nonpositive_polarity(case)] * case.b
    assert C.stated_nonpositive_polarity(case) > 0
    # sources outside the flow field: some in EVERY trip of the loops that count or skip them
    wev = C.warp_events(case)
    bad = C.source_out_of_range(wev)
    assert bad.sum(axis=1).tolist() == [len(C.oor_indices(case.n))] * case.b and bad[:, C.oor_indices(case.n)].all()
    for kernel in ("warp_dense_kernel", "warp_dense_bwd_kernel"):
        per_trip = C.oor_per_trip(case.n, kernel)
        assert len(per_trip) >= 2 and min(per_trip) > 0 and sum(per_trip) == len(C.oor_indices(case.n))
    t = wev[..., 2].astype(np.float64)
    if case.mixed_t:
        wave = LIM["time_range_kernel"][0] * LIM["time_range_kernel"][1]
        assert (t.min(axis=1) < 0).all() and (t.max(axis=1) > 0).all()
        assert (wave <= t.argmin(axis=1)).all() and (t.argmin(axis=1) < 2 * wave).all() and (t.argmax(axis=1) >= 2 * wave).all()
    else:
        assert (np.diff(t, axis=1) >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def first_trip(kernel, items):
    return C.trips(items, *LIM[kernel])[2]


def misses(err, dtype, what):
    return err >= FACTOR * C.bar(dtype, what)


@pytest.mark.parametrize("case", [BIG32, BIG64], ids=lambda c: c.id)
def test_events_of_the_first_trip_alone_miss_every_bar(case):
    """The oracle on the first grid x block events only, against the oracle on all of them."""
    b, n, pad = case.b, case.n, case.pad
    ev, wt, up_img, up_ev = C.splat_events(case), C.weights_of(case), C.upstream_image(case), C.upstream_events(case)
    # splat forward: the events of later trips do not vote
    m = first_trip("splat_kernel", n)
    assert misses(C.rel(C.ref_splat(ev[:, :m], pad, wt[:, :m]), C.ref_splat(ev, pad, wt)), case.dtype, "image")
    assert misses(C.rel(C.ref_count(ev[:, :m], pad), C.ref_count(ev, pad)), case.dtype, "image")
    # splat backward: the events of later trips get no gradient
    m = first_trip("splat_bwd_kernel", n)
    de, dw = C.ref_splat_backward(ev, pad, wt, up_img)
    de_cut, dw_cut = de.copy(), dw.copy()
    de_cut[:, m:], dw_cut[:, m:] = 0.0, 0.0
    assert misses(C.rel(de_cut, de), case.dtype, "grad") and misses(C.rel(dw_cut, dw), case.dtype, "grad")
    # warps: bit-exact bars -- any event of a later trip that moves is a miss; thousands do
    wev, flow = C.warp_events(case), C.flow_of(case)
    warped, bad = C.ref_warp_dense(wev, flow, "middle", True)
    m = first_trip("warp_dense_kernel", n)
    assert (warped[:, m:] != wev[:, m:]).any(axis=-1).sum() > 1000
    # warp backward: d_flow without the later trips; d_theta likewise, and without every trip but the first of each thread
    m = first_trip("warp_dense_bwd_kernel", n)
    dflow = C.ref_warp_dense_backward(wev, flow, "middle", True, up_ev)
    cut = up_ev.copy()
    cut[:, m:] = 0.0
    assert misses(C.rel(C.ref_warp_dense_backward(wev, flow, "middle", True, cut), dflow), case.dtype, "grad")
    m = first_trip("warp_2dof_bwd_kernel", n)
    theta = np.array([2.5, -1.5])
    dth = C.ref_warp_2dof_backward(wev[0], theta, "middle", True, up_ev[0])
    cut = up_ev[0].copy()
    cut[:m] = 0.0          # an accumulator that restarted each trip keeps the LAST trip only
    assert misses(C.rel(C.ref_warp_2dof_backward(wev[0], theta, "middle", True, cut), dth), case.dtype, "grad")
    cut = up_ev[0].copy()
    cut[m:] = 0.0
    assert misses(C.rel(C.ref_warp_2dof_backward(wev[0], theta, "middle", True, cut), dth), case.dtype, "grad")
    # time range (exact): the extremes of the first trip alone are not the row's
    m = first_trip("time_range_kernel", n)
    t = wev[..., 2]
    assert (t[:, :m].max(axis=1) != t.max(axis=1)).all()


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
def test_pixels_of_the_first_trip_alone_miss_every_bar(dtype):
    h, w = C.PIXEL_IMAGE
    x = C.images(1, C.PIXEL_IMAGE, dtype)
    for name, kernel in (("var", "variance_grad_kernel"), ("gm", "gradmag_grad_kernel")):
        _, grad = C.ref_cost(name, x, False, C.upstream_costs(1, dtype))
        cut = grad.copy().reshape(-1)
        cut[first_trip(kernel, h * w):] = 0.0
        assert misses(C.rel(cut, grad.reshape(-1)), dtype, "grad"), name
    # one blur pass (the others differ in the operator alone): forward against the image bar, adjoint against the gradient bar
    A = C.gauss_operator(w, C.gauss_taps(1), 1)
    for kernel, op, what in (("gauss1d_kernel", A, "image"), ("gauss1d_bwd_kernel", A.T, "grad")):
        y = C.apply_along(op, x[0], 1)
        cut = y.copy().reshape(-1)
        cut[first_trip(kernel, h * w):] = 0.0
        assert misses(C.rel(cut, y.reshape(-1)), dtype, what), kernel


@pytest.mark.parametrize("omit", [False, True])
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
def test_rows_and_columns_of_the_first_trip_alone_miss_the_cost_bars(dtype, omit):
    """The cost of the region's first kCostGrid rows and first kCostBlock columns, against the cost of the region."""
    x = C.images(3, C.COST_IMAGE, dtype)
    o = int(omit)
    for name in ("var", "gm"):
        full, _ = C.ref_cost(name, x, omit)
        for sub in (x[:, :o + LIM["kCostGrid"] + o, :], x[:, :, :o + LIM["kCostBlock"] + o]):
            if name == "gm" and not omit:
                # (the Sobel of the cut image would replicate the cut edge: cut the MAGNITUDE, as a kernel that dropped rows would)
                mags = [(O.sobel3(C.T64(x[k])) / 8.0).pow(2).sum(0).numpy() for k in range(3)]
                part = np.array([m[:sub.shape[1], :sub.shape[2]].mean() for m in mags])
            elif name == "gm":
                mags = [(O.sobel3(C.T64(x[k])) / 8.0).pow(2).sum(0).numpy()[1:-1, 1:-1] for k in range(3)]
                part = np.array([m[:sub.shape[1] - 2, :sub.shape[2] - 2].mean() for m in mags])
            else:
                part, _ = C.ref_cost(name, sub, omit)
            assert (np.abs(part - full) >= FACTOR * C.bar(dtype, "cost") * np.abs(full)).all(), (name, part, full)


# ---------------------------------------------------------------------------------------------------------------- the oracle's two forms
def test_oracle_agrees_with_itself_on_a_big_case():
    case = BIG64
    ev = C.splat_events(case)[0]
    wt = C.weights_of(case)[0]
    a = O.bilinear_vote_numpy(ev, C.padded(case.pad), (case.pad, case.pad), wt, eps=O.EPS_TORCH)
    b = O.bilinear_vote_torch(torch.from_numpy(ev), C.padded(case.pad), (case.pad, case.pad), torch.from_numpy(wt)).numpy()
    assert C.rel(a, b) <= 1e-12
    wev = C.warp_events(case)[0]
    wev = wev[~C.source_out_of_range(wev)]      # (the numpy form indexes rows and columns, the torch form the flattened image)
    flow = C.flow_of(case)[0]
    for direction, norm in (("middle", True), (0.25, False)):
        a = O.warp_dense_numpy(wev, flow, direction, norm)
        b = O.warp_dense_torch(torch.from_numpy(wev), torch.from_numpy(flow), direction, norm).numpy()
        assert C.rel(a, b) <= 1e-12
