"""GPU tests of the second-order contrast kernels on EVERY built (tile_h, tile_w, halo): the tangent forward with its slab and combine
route and its atomic flush, the owner product, ``EventPlan.iwe_dense_jvp`` / ``contrast_dense_hvp`` and the solver's Newton-CG /
trust-ncg on the tile the solver picks by itself.  tests/test_gpu_hvp.py runs one geometry (37 x 70, plan tile (32, 32), float64
windows); here the windows of tests/_hvp_tile_cases.py give every tile shape interior tiles, four-window corners, overhang on both
axes, whole empty tiles, halos larger than the tile, float32 windows and launches of exactly 163 840 B of LDS.

Yardsticks: CPU, float64, ``torch.autograd.functional.jvp`` / ``hvp``.  Bars are the project's (tests/test_gpu_hvp.py): images
relative L2 < 1e-4, values relative < 1e-5, ``d_flow`` and ``hv`` relative L2 < 1e-3.  Every image / gradient / product comparison
also holds PER CELL, max |got - want| <= bar * max |want| with the bar of its L2 form: a 5 % slip in one of 9 450 cells moves the
global L2 by 5e-4 only, a seam row or a corner cell must fail on its own.

What float32 arithmetic alone does to the per-cell form (``closed_form`` in float32 on the CPU against the float64 yardstick, main
window, amp 6; pinned by tests/test_hvp.py::test_per_cell_bars_hold_ten_times_over_in_float32): IWE 2.4e-6, tangent 2.6e-6 (bar
1e-4); d_flow 6.2e-6, hv 3.4e-6 (bar 1e-3) -- 38 to 290 times inside the bars.  On the runs window every constructed pixel's own
(d_flow, hv) lies within 1.4e-5 of the yardstick, relative to that pixel's own vector (bar 1e-3).

Measured on an MI355X (DESIGN 4.30 has the table): every triple, float64 or float32 windows alike, tangent 7.3e-7 - 7.6e-7 L2 and
1.0e-6 per cell, IWE 4.3e-7 - 4.4e-7 and 1.0e-6; through the spill path at most 1.4e-6 / 2.2e-6.  The launches of exactly 163 840 B
are accepted.  Float32 windows repeated the first call's bits in 0 of 10 calls, float64 windows always.  Owner product on the
constructed runs: d_flow <= 1.0e-6 L2, hv <= 6.3e-7, worst pixel against its own vector 2.0e-5.  Two Newton-CG estimates on the
solver's own tile (64, 64) are bit-identical; on tile (32, 64), float32 windows, they ended 1.9e-6 px apart, so the solver refuses
that tile (last test).  Every test prints what the kernels give."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hvp_tile_cases as T  # noqa: E402
from _hvp_tile_cases import G, MAIN, TINY, per_cell, rel  # noqa: E402

pytestmark = pytest.mark.gpu

BUILT = ((64, 64, 32), (32, 64, 32), (32, 32, 32), (16, 64, 32), (64, 64, 16), (32, 32, 16), (32, 32, 8), (64, 64, 64), (32, 64, 48))
FLOAT32_CASES = {((64, 64, 32), 2), ((32, 64, 32), 2), ((32, 64, 48), 2), ((64, 64, 64), 1)}       # (triple, windows): ACC = float
AT_LIMIT_CASES = {((16, 64, 32), 2), ((32, 64, 48), 1), ((32, 64, 48), 2)}                         # 163 840 B of dynamic LDS
LDS_BYTES = 160 * 1024


def built_triples():
    """The library's own table where it is there to ask (collection must not need it), else the nine it is known to hold."""
    from event_based_bos_amd import _hip

    if os.path.exists(os.environ.get("EBOS_HIP_LIBRARY", _hip.LIB_PATH)):
        return tuple(_hip.tiled_configs())
    return BUILT


def tid(t):
    return "x".join(str(int(a)) for a in t)


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


_plans = {}


def plan_of(ebos, name, ev, shape, tile):
    """One plan per (window name, tile) for the module: the plan is read-only to every test but for its workspace cache."""
    key = (name, tuple(shape), tuple(tile))
    if key not in _plans:
        _plans[key] = T.plan_of(ebos, ev, shape, tile)
    return _plans[key]


def operands(shape, amp=6.0, seed=91):
    return G(T.flow_u(shape, amp), torch.float32), G(T.direction_v(shape, seed), torch.float32)


def fits_of(ebos):
    return ebos.load_library().ebos_iwe_multiref_fits


def check_image(what, got, want, bar, report):
    errs = (rel(got, want), per_cell(got, want))
    report.append(f"{what} L2 {errs[0]:.2e} cell {errs[1]:.2e}")
    assert bool(torch.isfinite(got).all()), what
    assert errs[0] < bar and errs[1] <= bar, (what, errs)


def events_beyond(ev, flow, triple):
    """How many events the tangent kernel of this triple hands to its spill path: the top-left tap outside rows / columns
    [0, L - 1) of the window of the event's source tile (the events keep 5e-4 px from every integer, so float32 decides alike)."""
    th, tw, hl = triple
    warped = T.O.warp_dense_numpy(ev, flow, "first", True)
    out = np.zeros(len(ev), dtype=bool)
    for axis, t in ((0, th), (1, tw)):
        cell = np.floor(warped[:, axis]) - ((ev[:, axis].astype(np.int64) // t) * t - hl)
        out |= (cell < 0) | (cell >= t + 2 * hl - 1)
    return int(out.sum())


def workspace(plan, halo, windows):
    return plan.__dict__["_workspaces"][("tangent", halo, windows)]


def slab_bytes(shape, triple, windows, fits):
    th, tw, hl = triple
    tiles = -(-shape[0] // th) * -(-shape[1] // tw)
    return tiles * windows * (th + 2 * hl) * (tw + 2 * hl) * (8 if fits == 2 else 4)


# ---------------------------------------------------------------------------------------------- the parametrization itself
def test_built_triples_hold_the_float32_and_the_at_limit_cases(ebos):
    from event_based_bos_amd import _hip

    fits = fits_of(ebos)
    assert set(built_triples()) == set(_hip.tiled_configs()) == set(BUILT)
    kinds = {(t, w): int(fits(*t, w)) for t in BUILT for w in (1, 2)}
    lds = {(t, w): w * (t[0] + 2 * t[2]) * (t[1] + 2 * t[2]) * (8 if k == 2 else 4) for (t, w), k in kinds.items() if k}
    assert {c for c, k in kinds.items() if k == 1} == FLOAT32_CASES
    assert {c for c, b in lds.items() if b == LDS_BYTES} == AT_LIMIT_CASES and max(lds.values()) == LDS_BYTES
    assert [c for c, k in kinds.items() if k == 0] == [((64, 64, 64), 2)]


# ---------------------------------------------------------------------------------------------- tangent forward, every triple
def run_triple(ebos, name, ev, shape, amp, triple, pads=(0, 2), repeats=10):
    """Every (windows, pad, route) of one triple against the yardstick -> the report lines.  Asserts the accumulator from ``fits``
    (and from the size of the slab workspace the library asked for), the bars in both forms and the bit claims."""
    from event_based_bos_amd import event_plan as EP

    th, tw, hl = triple
    fits = fits_of(ebos)
    plan = plan_of(ebos, (name, amp), ev, shape, (th, tw))
    flow, v = operands(shape, amp)
    spills = events_beyond(ev, T.flow_u(shape, amp), triple)
    lines = []
    tangents = {}
    for with_iwe in (True, False):
        windows = 2 if with_iwe else 1
        kind = int(fits(th, tw, hl, windows))
        if kind == 0:
            # the documented fall-back of ``_hvp_halo``: a built halo of the tile whose windows do fit, float64 first
            got_halo = EP._hvp_halo(plan, hl, windows, "test")
            assert (triple, windows) == ((64, 64, 64), 2) and got_halo == 16 and int(fits(th, tw, got_halo, windows)) == 2
            a = plan.iwe_dense_jvp(flow, v, halo=hl)
            b = plan.iwe_dense_jvp(flow, v, halo=got_halo)
            assert ("tangent", hl, windows) not in plan.__dict__["_workspaces"]
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            lines.append(f"  {windows} window(s): do not fit; halo {hl} falls back to halo {got_halo} (float64), the same bits")
            continue
        assert kind == (1 if (triple, windows) in FLOAT32_CASES else 2)
        assert EP._hvp_halo(plan, hl, windows, "test") == hl                          # a halo that fits is honoured
        acc = "float64" if kind == 2 else "float32"
        for pad in pads:
            want_iwe, want_tangent = T.ref_images((name, amp), ev, T.flow_u(shape, amp), T.direction_v(shape), pad)
            report = []
            for route, splits in (("slab", None), ("flush x2", 2)):
                iwe, tangent = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=hl, with_iwe=with_iwe, splits=splits)
                assert tangent.shape == (shape[0] + 2 * pad, shape[1] + 2 * pad) and tangent.dtype == torch.float32
                assert (iwe is not None) == with_iwe
                check_image(f"{route} tangent", tangent, want_tangent, 1e-4, report)
                if with_iwe:
                    check_image(f"{route} IWE", iwe, want_iwe, 1e-4, report)
                if route == "slab":
                    tangents[(with_iwe, pad)] = tangent
            assert workspace(plan, hl, windows).numel() == slab_bytes(shape, triple, windows, kind)
            lines.append(f"  {windows} window(s) {acc} ({windows * (th + 2 * hl) * (tw + 2 * hl) * (8 if kind == 2 else 4)} B LDS) pad {pad}: "
                         + "; ".join(report))
        if kind == 1:   # float32 windows: LDS float atomics in the order the hardware picks -- reported, not asserted
            first = plan.iwe_dense_jvp(flow, v, halo=hl, with_iwe=with_iwe)[1]
            same = sum(torch.equal(plan.iwe_dense_jvp(flow, v, halo=hl, with_iwe=with_iwe)[1], first) for _ in range(repeats))
            lines.append(f"  {windows} window(s) float32: {same} of {repeats} repeated slab calls repeat the first call's bits")
    both64 = int(fits(th, tw, hl, 1)) == 2 and int(fits(th, tw, hl, 2)) == 2
    for pad in pads:
        if (True, pad) in tangents and (False, pad) in tangents:
            equal = torch.equal(tangents[(True, pad)], tangents[(False, pad)])
            lines.append(f"  pad {pad}: tangent with / without the IWE bit-identical: {equal} (float64 both: {both64}, events beyond the halo: {spills})")
            if both64 and spills == 0:   # the same float64 windows, summed by the combine pass in the same order
                assert equal
            assert rel(tangents[(False, pad)], tangents[(True, pad)]) < 1e-4
    return lines


@pytest.mark.parametrize("triple", built_triples(), ids=tid)
def test_tangent_of_every_built_triple(ebos, triple):
    ev = T.kink_free(MAIN, 6.0)
    assert events_beyond(ev, T.flow_u(MAIN, 6.0), tuple(triple)) == 0                 # amp 6 stays inside every built halo
    lines = run_triple(ebos, "kf", ev, MAIN, 6.0, tuple(triple))
    print(f"tile {triple[:2]} halo {triple[2]} at {MAIN}, amp 6:\n" + "\n".join(lines))


# amp 12 leaves halo 8 (the spill path carries events there; halos 16 and 32 still hold every event); amp 40 leaves halos 16 and 32 as
# well, so that the spill path also runs beside the 96 x 96 windows of the solver's default tile and beside float32 windows
SPILL_CASES = [(12.0, (32, 32, 8)), (12.0, (64, 64, 16)), (12.0, (64, 64, 32)), (40.0, (64, 64, 16)), (40.0, (32, 64, 32))]


@pytest.mark.parametrize("amp,triple", SPILL_CASES, ids=[f"amp{int(a)}-{tid(t)}" for a, t in SPILL_CASES])
def test_tangent_with_events_beyond_the_halo(ebos, amp, triple):
    ev, flow = T.kink_free(MAIN, amp), T.flow_u(MAIN, amp)
    warped = T.O.warp_dense_numpy(ev, flow, "first", True)
    assert (np.abs(warped[:, :2] - ev[:, :2]).max(1) > 9).sum() > 100                 # the case does leave the 8-pixel halo
    beyond = events_beyond(ev, flow, triple)
    if amp == 40.0 or triple[2] == 8:   # (at amp 40 most of the far events leave the image, not only the window)
        assert beyond > (100 if triple[2] < 32 else 50)
    lines = run_triple(ebos, "kf", ev, MAIN, amp, triple, pads=(0, 2), repeats=3)
    print(f"tile {triple[:2]} halo {triple[2]} at {MAIN}, amp {amp:g}, {beyond} events beyond the halo:\n" + "\n".join(lines))


@pytest.mark.parametrize("splits", [1, 3, 64])
def test_flush_route_work_items(ebos, splits):
    """k work items per tile on the atomic flush; with 64, most items of a tile hold no event (a chunk is a multiple of 64 events)."""
    ev = T.kink_free(MAIN, 6.0)
    plan = plan_of(ebos, "kf", ev, MAIN, (64, 64))
    flow, v = operands(MAIN)
    report = []
    for pad in (0, 2):
        want_iwe, want_tangent = T.ref_images(("kf", 6.0), ev, T.flow_u(MAIN), T.direction_v(MAIN), pad)
        iwe, tangent = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=16, splits=splits)
        _, alone = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=16, splits=splits, with_iwe=False)
        check_image(f"pad {pad} IWE", iwe, want_iwe, 1e-4, report)
        check_image(f"pad {pad} tangent", tangent, want_tangent, 1e-4, report)
        check_image(f"pad {pad} tangent alone", alone, want_tangent, 1e-4, report)
    print(f"(64, 64, 16), {splits} work item(s) per tile: " + "; ".join(report))


# ---------------------------------------------------------------------------------------------- empty tiles, poisoned workspace
def empty_tiles(plan):
    tile_px = int(plan.tile[0]) * int(plan.tile[1])
    at = plan.key_offsets[::tile_px].cpu()
    return [i for i in range(len(at) - 1) if int(at[i]) == int(at[i + 1])]


def test_every_tile_shape_has_a_whole_empty_tile(ebos):
    ev = T.empty_tiles_window()
    for tile in T.PLAN_TILES:
        plan = plan_of(ebos, "empty", ev, MAIN, tile)
        n_tiles = -(-MAIN[0] // tile[0]) * -(-MAIN[1] // tile[1])
        empty = empty_tiles(plan)
        print(f"tile {tile}: tiles without events {empty} of {n_tiles}")
        assert 1 <= len(empty) < n_tiles


@pytest.mark.parametrize("triple", [(64, 64, 16), (32, 64, 48), (16, 64, 32)], ids=tid)
def test_combine_pass_reads_no_slab_that_was_not_written(ebos, triple):
    """The slab workspace is not zero-filled and a tile without events writes no slab: with the workspace set to 0xFF bytes (NaN
    as float64 and as float32) between two calls, no output cell may change or stop being finite."""
    th, tw, hl = triple
    ev = T.empty_tiles_window()
    plan = plan_of(ebos, "empty", ev, MAIN, (th, tw))
    assert empty_tiles(plan)
    flow, v = operands(MAIN)
    fits = fits_of(ebos)
    for with_iwe in (True, False):
        windows = 2 if with_iwe else 1
        kind = int(fits(th, tw, hl, windows))
        assert kind != 0
        for pad in (0, 2):
            want_iwe, want_tangent = T.ref_images(("empty", 6.0), ev, T.flow_u(MAIN), T.direction_v(MAIN), pad)
            first = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=hl, with_iwe=with_iwe)
            ws = workspace(plan, hl, windows)
            assert ws.dtype == torch.uint8 and ws.numel() == slab_bytes(MAIN, triple, windows, kind)
            ws.fill_(0xFF)
            assert bool(torch.isnan(ws.view(torch.float64 if kind == 2 else torch.float32)).all())
            second = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=hl, with_iwe=with_iwe)
            assert workspace(plan, hl, windows) is ws
            report = []
            check_image("tangent", second[1], want_tangent, 1e-4, report)
            if with_iwe:
                check_image("IWE", second[0], want_iwe, 1e-4, report)
            same = torch.equal(second[1], first[1]) and (not with_iwe or torch.equal(second[0], first[0]))
            print(f"{triple} {windows} window(s) {'float64' if kind == 2 else 'float32'} pad {pad}, poisoned workspace: " + "; ".join(report)
                  + f"; bits of the first call: {same}")
            if kind == 2:
                assert same


# ---------------------------------------------------------------------------------------------- a window smaller than a tile
TINY_CASES = [((32, 32, 8), True), ((64, 64, 16), True), ((64, 64, 64), False)]


@pytest.mark.parametrize("triple,with_iwe", TINY_CASES, ids=[tid(t) for t, _ in TINY_CASES])
def test_tiny_window(ebos, triple, with_iwe):
    """13 x 21, smaller than every tile and every halo: the yardstick's images, and nothing written outside them (both entries add
    into caller-zeroed images inside a NaN-guarded buffer)."""
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    th, tw, hl = triple
    H, W = TINY
    ev = T.kink_free(TINY)
    plan = plan_of(ebos, "tiny", ev, TINY, (th, tw))
    flow, v = operands(TINY)
    windows = 2 if with_iwe else 1
    kind = int(fits_of(ebos)(th, tw, hl, windows))
    assert kind == (1 if (triple, windows) in FLOAT32_CASES else 2)
    lib = ebos.load_library()
    for pad in (0, 2):
        want_iwe, want_tangent = T.ref_images(("tiny", 6.0), ev, T.flow_u(TINY), T.direction_v(TINY), pad)
        report = []
        iwe, tangent = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=hl, with_iwe=with_iwe)
        check_image("slab tangent", tangent, want_tangent, 1e-4, report)
        if with_iwe:
            check_image("slab IWE", iwe, want_iwe, 1e-4, report)
        h, w = H + 2 * pad, W + 2 * pad
        guard = 4096
        for entry in ("flush", "slab"):
            big = torch.full((guard + 2 * h * w + guard,), float("nan"), dtype=torch.float32, device=T.dev())
            big[guard:guard + 2 * h * w] = 0.0
            t_at, i_at = big[guard:guard + h * w], big[guard + h * w:guard + 2 * h * w]
            if entry == "flush":
                check(lib.ebos_iwe_dense_tangent_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow), ptr(v),
                                                           H, W, th, tw, hl, 1, pad, pad, ptr(i_at) if with_iwe else None, ptr(t_at), stream_ptr()),
                      "tangent")
            else:
                ws = torch.full((int(lib.ebos_iwe_tangent_slab_workspace_bytes(H, W, th, tw, hl, windows)),), 0xFF, dtype=torch.uint8, device=T.dev())
                check(lib.ebos_iwe_dense_tangent_slab_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow), ptr(v),
                                                          H, W, th, tw, hl, pad, pad, ptr(ws), ws.numel(), ptr(i_at) if with_iwe else None,
                                                          ptr(t_at), stream_ptr()), "tangent slab")
            torch.cuda.synchronize()
            assert bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[-guard:]).all()), entry
            check_image(f"guarded {entry} tangent", t_at.reshape(h, w), want_tangent, 1e-4, report)
            if with_iwe:
                check_image(f"guarded {entry} IWE", i_at.reshape(h, w), want_iwe, 1e-4, report)
            else:
                assert int(torch.count_nonzero(i_at)) == 0                             # the IWE's place stays as the caller left it
        print(f"{TINY} {triple} {windows} window(s) {'float64' if kind == 2 else 'float32'} pad {pad}: " + "; ".join(report))


# ---------------------------------------------------------------------------------------------- owner product, run lengths
def check_product(what, got, want, shape, only=None):
    value, d_flow, hv = got
    errs = (abs(float(value) - want[0]) / abs(want[0]), rel(d_flow, want[1]), rel(hv, want[2]), per_cell(d_flow, want[1]), per_cell(hv, want[2]))
    print(f"{what}: value rel {errs[0]:.2e}, d_flow L2 {errs[1]:.2e} cell {errs[3]:.2e}, hv L2 {errs[2]:.2e} cell {errs[4]:.2e}")
    assert value.dim() == 0 and d_flow.shape == hv.shape == (2,) + tuple(shape) and d_flow.dtype == hv.dtype == torch.float32
    assert bool(torch.isfinite(d_flow).all()) and bool(torch.isfinite(hv).all())
    assert errs[0] < 1e-5 and errs[1] < 1e-3 and errs[2] < 1e-3 and errs[3] <= 1e-3 and errs[4] <= 1e-3
    if only is not None:   # the constructed pixels among themselves, and each against its own vector: no pixel hides behind another
        worst = {}
        for name, g, w in (("d_flow", d_flow.cpu().numpy().astype(np.float64), want[1]), ("hv", hv.cpu().numpy().astype(np.float64), want[2])):
            among = np.abs(g[:, only] - w[:, only]).max() / np.abs(w[:, only]).max()
            own = max(np.linalg.norm(g[:, r, c] - w[:, r, c]) / np.linalg.norm(w[:, r, c]) for r, c in T.CONSTRUCTED)
            worst[name] = (among, own)
            assert among <= 1e-3 and own < 1e-3, (what, name, among, own)
        print("    constructed pixels: " + ", ".join(f"{k} cell {a:.2e}, worst pixel against its own vector {o:.2e}" for k, (a, o) in worst.items()))
    return errs


PRODUCT_CASES = (("image_variance", False, 0, 0.0), ("image_variance", True, 2, 0.0), (T.TWO_COSTS, False, 0, 1.0), (T.TWO_COSTS, True, 2, 1.0))


@pytest.mark.parametrize("tile", T.PLAN_TILES, ids=tid)
def test_owner_product_on_constructed_runs(ebos, tile):
    """Runs of exactly 1 .. 5, 63 / 64 / 65 and 127 / 128 / 129 events, two 300-event pixels in adjacent lanes of one wave and one on
    the last in-image key of the overhanging corner tile: every path of the owner kernel, pixel by pixel."""
    from event_based_bos_amd import event_plan as EP
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    ev = T.runs_window()
    plan = plan_of(ebos, "runs", ev, MAIN, tile)
    counts = plan.pixel_event_counts().cpu()
    assert {p: int(counts[p]) for p in T.CONSTRUCTED} == T.CONSTRUCTED and int(counts.sum()) == len(ev) == plan.n
    flow, v = operands(MAIN)
    only = T.constructed_mask()
    halo = EP._hvp_halo(plan, "auto", 2, "test")
    kind = int(fits_of(ebos)(tile[0], tile[1], halo, 2))
    print(f"plan tile {tile}: halo {halo}, two {'float64' if kind == 2 else 'float32'} windows")
    for cost, omit, pad, blur in PRODUCT_CASES:
        want = T.ref_hvp("runs", ev, T.flow_u(MAIN), T.direction_v(MAIN), cost, omit, pad, blur)
        got = plan.contrast_dense_hvp(flow, v, dict(cost) if isinstance(cost, dict) else cost, omit, blur, pad=(pad, pad))
        assert got[3]["halo"] == halo
        check_product(f"  {cost} omit={omit} pad={pad} blur={blur}", got[:3], want, MAIN, only)
    # the owner entry on one pair of upstream images, into NaN-filled outputs: the same bits, no NaN left, zeros on empty pixels
    iwe, tangent = plan.iwe_dense_jvp(flow, v)
    affine = torch.tensor([0.37, -0.11, 0.21, 0.05], dtype=torch.float32, device=T.dev())
    outs = []
    for _ in range(2):
        d_flow, hv = (torch.full((2,) + MAIN, float("nan"), dtype=torch.float32, device=T.dev()) for _ in range(2))
        check(ebos.load_library().ebos_iwe_dense_hvp_owner_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow),
                                                                   ptr(v), MAIN[0], MAIN[1], tile[0], tile[1], 0, 0, ptr(iwe), ptr(tangent),
                                                                   ptr(affine), 0, ptr(d_flow), ptr(hv), stream_ptr()), "owner")
        outs.append((d_flow, hv))
    launched = EP._launch_hvp_owner(plan, flow, v, (0, 0), iwe, tangent, affine, 0, True)
    for a, b in ((outs[0], outs[1]), (outs[0], launched)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                    # (NaN would not compare equal)
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())
    empty = plan.pixel_event_counts() == 0
    assert int(empty.sum()) > 0 and int(torch.count_nonzero(outs[0][0][:, empty])) == 0 and int(torch.count_nonzero(outs[0][1][:, empty])) == 0
    assert int(torch.count_nonzero(outs[0][1][:, ~empty])) > 0


# ---------------------------------------------------------------------------------------------- full product, default route
STATE_CASES = (("image_variance", 0.0), (dict(T.TWO_COSTS), 1.0))


def test_product_on_the_default_route(ebos):
    """Tile (64, 64), halo "auto" -- what the solver runs: halo 16 with the IWE and, from the state, halo 16 without it; float64
    windows in both calls, so ``hv`` from a reused state is the product without one bit for bit, and ten repeats repeat their bits."""
    ev = T.kink_free(MAIN)
    plan = T.plan_of(ebos, ev, MAIN, (64, 64))                                        # (its own plan: the workspace keys are read below)
    flow, v = operands(MAIN)
    w = G(T.direction_v(MAIN, 92), torch.float32)
    fits = fits_of(ebos)
    for cost, blur in STATE_CASES:
        want = T.ref_hvp(("kf", 6.0), ev, T.flow_u(MAIN), T.direction_v(MAIN), cost, False, 0, blur)
        value, d_flow, hv, state = plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur)
        check_product(f"{cost} blur={blur}", (value, d_flow, hv), want, MAIN)
        assert state["halo"] == 16 and fits(64, 64, 16, 2) == 2 and fits(64, 64, 16, 1) == 2
        hv2 = plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur, state=state)[2]
        keys = sorted(k for k in plan.__dict__["_workspaces"] if k[0] == "tangent")
        assert keys == [("tangent", 16, 1), ("tangent", 16, 2)]                       # the tangent alone ran at the state's halo
        again = [torch.equal(plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur)[2], hv) for _ in range(10)]
        print(f"    hv with the reused state, bits equal: {torch.equal(hv2, hv)}; ten more products, bits equal: {sum(again)} of 10")
        assert torch.equal(hv2, hv) and all(again)
        hw = plan.contrast_dense_hvp(flow, w, cost, blur_sigma=blur, state=state)[2]
        want_w = T.ref_hvp(("kf", 6.0), ev, T.flow_u(MAIN), T.direction_v(MAIN, 92), cost, False, 0, blur)
        a, b = float((w.double() * hv.double()).sum()), float((v.double() * hw.double()).sum())
        print(f"    second direction: hv L2 {rel(hw, want_w[2]):.2e} cell {per_cell(hw, want_w[2]):.2e}; <w, Hv> = {a:.6e}, <v, Hw> = {b:.6e}, "
              f"relative difference {abs(a - b) / abs(a):.2e}")
        assert rel(hw, want_w[2]) < 1e-3 and per_cell(hw, want_w[2]) <= 1e-3 and abs(a - b) < 1e-3 * abs(a)


# ---------------------------------------------------------------------------------------------- solver
def make_solver(ebos, cfg):
    return ebos.solver.ContrastMaximization(MAIN, MAIN, solver_config=cfg)


def estimate_from_start(ebos, cfg, ev, start):
    slv = make_solver(ebos, cfg)
    slv.previous_best = start.copy()
    flow = slv.estimate(ev)
    return slv, flow


@pytest.mark.parametrize("method", ["Newton-CG", "trust-ncg"])
def test_solver_on_its_default_tile(ebos, method):
    """No ``tile`` key: the hessp methods plan on (64, 64) and run halo 16 -- float64 windows with and without the IWE."""
    from event_based_bos_amd.solver import contrast_maximization as CM

    ev = T.solver_events()
    cfg = T.solver_config(method)
    assert "tile" not in cfg
    slv = make_solver(ebos, cfg)
    plan = slv._build_plan(ev)
    assert tuple(plan.tile) == tuple(slv.plan_tile()) == CM.MULTI_REFERENCE_TILE == (64, 64) and not plan.lean
    p = np.random.RandomState(93).standard_normal(T.theta_start().shape)
    l_ref, g_ref, hp_ref = T.ref_loss_hvp(ev, p)
    value_and_grad, hessp = slv._hessp_objective(plan, T.PATCH, T.PATCH, None)
    theta = torch.from_numpy(T.theta_start()).double()
    loss, grad = value_and_grad(theta)
    hp = hessp(theta, torch.from_numpy(p))
    errs = (abs(float(loss) - l_ref) / abs(l_ref), rel(grad, g_ref), rel(hp, hp_ref), per_cell(grad, g_ref), per_cell(hp, hp_ref))
    print(f"{method}: loss rel {errs[0]:.2e}, d_theta L2 {errs[1]:.2e} cell {errs[3]:.2e}, H p L2 {errs[2]:.2e} cell {errs[4]:.2e}")
    assert slv.hessp_calls == 1 and errs[0] < 1e-5 and max(errs[1:]) < 1e-3
    assert sorted(k for k in plan.__dict__["_workspaces"] if k[0] == "tangent") == [("tangent", 16, 1), ("tangent", 16, 2)]
    runs = [estimate_from_start(ebos, cfg, ev, T.theta_start()) for _ in range(2)]
    s0, flow = runs[0]
    with torch.no_grad():
        start = T.ref_loss(torch.from_numpy(T.theta_start()).double(), ev).item()
        final = T.ref_loss(s0.patch_flow.detach().cpu().double(), ev).item()
    same = torch.equal(runs[0][0].patch_flow, runs[1][0].patch_flow)
    print(f"    {s0.history[0]:.5f} -> {float(s0.scipy_result.fun):.5f} in {len(s0.history)} evaluations and {s0.hessp_calls} products; float64 loss "
          f"{start:.5f} -> {final:.5f}; two estimates from the same start, patch_flow bits equal: {same}")
    assert s0.loop_mode == "hessp" and flow.shape == (2,) + MAIN and np.isfinite(flow).all()
    assert s0.hessp_calls >= 1 and float(s0.scipy_result.fun) < s0.history[0] and final < start
    assert same


def test_newton_cg_yaml_on_its_own_tile(ebos):
    import yaml

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "cmax_newton_cg.yaml")))["solver"]
    assert cfg["optimizer"]["method"] == "Newton-CG" and "tile" not in cfg
    cfg["optimizer"]["n_iter"] = 3
    slv = make_solver(ebos, cfg)
    gh, gw = T.O.patch_grid_shape(MAIN, slv.patch_size, slv.sliding_window)
    slv.previous_best = np.full((2, gh, gw), 0.5, dtype=np.float32)
    ev = T.solver_events()
    assert tuple(slv._build_plan(ev).tile) == (64, 64)
    flow = slv.estimate(ev)
    print(f"configs/cmax_newton_cg.yaml at {MAIN}: {slv.history[0]:.5f} -> {min(slv.history):.5f}, {slv.hessp_calls} products")
    assert slv.loop_mode == "hessp" and flow.shape == (2,) + MAIN and np.isfinite(flow).all() and np.isfinite(slv.history).all()
    assert slv.hessp_calls >= 1 and min(slv.history) < slv.history[0]


def test_solver_on_a_tile_with_float32_windows(ebos):
    """``tile: [32, 64]``: both built halos keep the two windows of a product's first call as float32 only, so the IWE behind the
    loss and the gradient is summed by LDS float atomics in the order the hardware picks (the tangent alone, one window of halo
    48, is float64).  Measured on an MI355X with this window before the refusal existed: of 10 repeated
    ``contrast_dense_hvp(dense, 0)`` the value repeated its bits 10 times, ``d_flow`` 0 times, and two Newton-CG estimates of 4
    iterations from the same start ended 1.9e-6 px apart (6 evaluations and 4 products each) -- the amplification DESIGN 4.30
    describes.  The hessp methods therefore refuse such a tile at construction, naming the tiles that work; the plan operators
    still run it (tests above) and this test prints their repeat counts."""
    from event_based_bos_amd import event_plan as EP

    ev = T.solver_events()
    fits = fits_of(ebos)
    assert EP.hvp_tile_halo((32, 64), "auto", 2, "test") == (48, 1) and fits(32, 64, 32, 2) == 1 and fits(32, 64, 48, 1) == 2
    for method in ("Newton-CG", "trust-ncg", "trust-krylov"):
        with pytest.raises(NotImplementedError, match=r"tile \[32, 64\].*float32.*\[16, 64\], \[32, 32\], \[64, 64\]"):
            make_solver(ebos, T.solver_config(method, tile=(32, 64)))
    with pytest.raises(NotImplementedError, match=r"tile \[64, 64\], halo 32.*float32"):
        make_solver(ebos, T.solver_config("Newton-CG", tile=(64, 64), halo=32))
    assert make_solver(ebos, T.solver_config("Adam", tile=(32, 64))).tile == (32, 64)  # (the first-order methods take any tile)
    for tile in ((16, 64), (32, 32), (64, 64)):
        assert tuple(make_solver(ebos, T.solver_config("Newton-CG", tile=tile)).plan_tile()) == tile
    plan = plan_of(ebos, "solver", ev, MAIN, (32, 64))
    dense, zero = G(T.dense_of(torch.from_numpy(T.theta_start()).double()).numpy(), torch.float32), torch.zeros((2,) + MAIN, device=T.dev())
    first = plan.contrast_dense_hvp(dense, zero)
    again = [plan.contrast_dense_hvp(dense, zero) for _ in range(10)]
    assert first[3]["halo"] == 48
    print(f"tile (32, 64), halo 48, two float32 windows: of 10 repeated calls, value bits equal {sum(torch.equal(a[0], first[0]) for a in again)}, "
          f"d_flow bits equal {sum(torch.equal(a[1], first[1]) for a in again)}, d_flow rel L2 between calls "
          f"{max(rel(a[1], first[1]) for a in again):.2e}")
