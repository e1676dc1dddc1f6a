"""The event loop of the tile-private backward kernel (csrc/iwe_tile_core.h: bwd_compact_slice, bwd_sweeps_mode, bwd_lean_sweeps, the
set-up around BwdPre) where such a loop breaks: at the seams between chunks, not at scale.  A chunk is 64 groups of 4 events, a
workgroup has 16 waves, chunks 0 .. 31 are pre-assigned and everything past 8192 events of a work item is drawn from an LDS counter;
the fixed-point main sweep rotates three register sets (the third one runs only when a wave takes a third chunk), the queue is reset
before the spill sweep, before the exact f64 redo and in the forward redo, and the first two chunks of a wave are requested early.
The windows of tests/_bwd_loop_cases.py (pinned on the CPU by tests/test_bwd_loop_cases.py) put 0 .. 24 577 events into the four
tiles of a 2 x 2-tile image: every other backward test of the suite stays below 8192 events per work item, where no draw from the
queue is live and none of the three resets can be observed.

Yardsticks -- the code under test is never its own: (i) the general global-atomic kernels on the same float32 inputs (halo=None on a
full plan); (ii) float64 autograd of oracle.ebos_oracle on the CPU.  Bars: whole image rel-L2 < 2e-5 against (i), < 1e-3 against (ii)
for the variance cost (the bars of test_backward_fixed_point_scatter_is_exact_or_redone_in_f64); per tile T, on the given-upstream
path,  ||got_T - want_T|| <= 2e-5 ||want_T|| + (u / 2) sqrt(2 sum count^2),  u = 2^-20 x 2 dt_bound max |upstream|  -- the largest unit
bwd_fx_unit can choose at 21 bits, every event rounded to nearest once per component (a pixel's gradient depends on its own events
only, so one lost event of a small tile cannot hide in the image norm).  Two runs of a fixed-point route are equal bit for bit.

Largest errors observed on an MI355X (whole image rel-L2 against (i); worst tile as a fraction of its bar):
    1  lean sweep, built halos   8.6e-07; 0.14 of the bar (the one-event tile of set a)      run-time windows   5.5e-07; 0.03
    2  variance cost             3.4e-06 against (i), 3.5e-06 against (ii); the variance itself 3e-08 against (ii)
    3  spill sweep               4.9e-07; 0.02; the spilling row on its own 7.1e-07
    4  f64 redo                  "before" plans 4.5e-07; 0.02 (variance job 2.6e-06); upstream spike 6.2e-08, the source pixels that
                                 do not touch the spike on their own 3.5e-07
    5  hot-pixel tile            3.0e-07; 0.02; the hot tile on its own 1.3e-07
    6  plans that are not lean   5.9e-08; 0.004; d_weight equal to the general kernels'; 1.7e-07 against (ii)
    7  forward redo              images bit for bit; NaN-flow image 2.1e-07 against (ii)
    8  grid route                d_theta 2.6e-07 against the dense route, 6.8e-07 against (ii); the resident launch ran (status 0)
    9  persistent batch          images bit for bit; 4.2e-07 against (ii)
Without the queue reset in front of the spill sweep (bwd_sweeps_mode; a scratch build, not committed) both cases of 3 and the
set-e case of the upstream spike fail -- tile 3 at 886 and 2708 times its bar, 1.3e-02 and 4.3e-02 of the whole image -- and every
older backward test of the suite still passes.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ebos_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bwd_loop_cases as B  # noqa: E402
from _bwd_loop_cases import MAIN, SETS, TRIPLES  # noqa: E402

pytestmark = pytest.mark.gpu

BAR_GENERAL, BAR_ORACLE = 2e-5, 1e-3
_plans, _wants = {}, {}


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def G(a, dtype=None):
    t = torch.from_numpy(np.asarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def rel(a, b):
    return O.rel_l2(a, b)


def plan_of(ebos, key, ev, size, tile, emit, direction="first"):
    k = (key, tile, emit, direction)
    if k not in _plans:
        _plans[k] = ebos.EventPlan.build(G(ev), size, direction, True, tile=tile, emit=emit)
    return _plans[k]


def grad_up(plan, flow, up, halo, splits=None, weight=None):
    """d (sum upstream . IWE) / d flow -- and d / d weight -- through ``iwe_dense(...).backward(gradient=upstream)``."""
    fg = flow.clone().requires_grad_(True)
    wg = None if weight is None else weight.clone().requires_grad_(True)
    plan.iwe_dense(fg, halo=halo, splits=splits, weight=wg).backward(gradient=up)
    return fg.grad if weight is None else (fg.grad, wg.grad)


def grad_cost(plan, flow, halo, omit=False, pad=(0, 0)):
    fg = flow.clone().requires_grad_(True)
    v = plan.contrast_dense(fg, "image_variance", omit_boundary=omit, pad=pad, halo=halo)
    value = v.item()
    v.backward()
    return value, fg.grad


def general_grad(ebos, key, ev, size, tile, fl, up, direction="first"):
    """Yardstick (i), once per case: the general kernels on a full plan."""
    k = (key, tuple(tile), direction)
    if k not in _wants:
        full = plan_of(ebos, key[0], ev, size, tile, "full", direction)
        assert not full.lean
        _wants[k] = grad_up(full, G(fl, torch.float32), G(up, torch.float32), None).cpu().numpy()
    return _wants[k]


def check(label, got, want, size, tile, ev, up_max, dt_bound=1.0):
    """Whole-image and per-tile bars against yardstick (i); prints what it saw."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    counts = B.pixel_counts(ev, size)
    whole = rel(got, want)
    rows = []
    ok = True
    for k, (rs, cs) in enumerate(B.tile_slices(size, tile)):
        err = float(np.linalg.norm(got[:, rs, cs].astype(np.float64) - want[:, rs, cs]))
        ref = float(np.linalg.norm(want[:, rs, cs].astype(np.float64)))
        bar = BAR_GENERAL * ref + B.allowance(counts[rs, cs], up_max, dt_bound)
        rows.append(f"tile {k} ({int(counts[rs, cs].sum())} ev): {err:.2e} / bar {bar:.2e} ({err / bar if bar else 0.0:.2f})")
        ok &= err <= bar
    print(f"[{label}] whole image rel-L2 {whole:.2e}; " + "; ".join(rows))
    assert np.isfinite(got).all()
    assert whole < BAR_GENERAL, label
    assert ok, label


def parts_of(plan):
    pt = plan.part_table.cpu().numpy()
    return tuple(int(v) for v in np.diff(pt[:5]))


def test_built_triples_are_the_ones_the_cases_name(ebos):
    tiles = {t[:2] for t in TRIPLES}
    assert sorted(t for t in ebos._hip.slab_configs() if t[:2] in tiles) == sorted(TRIPLES)


# ------------------------------------------------------------------------------------------ 1. lean sweep, given upstream
LEAN = [(MAIN, s) for s in "abcde"] + [(t, s) for t in TRIPLES[1:] for s in "de"]


@pytest.mark.parametrize("triple,name", LEAN, ids=["x".join(map(str, t)) + "-" + s for t, s in LEAN])
def test_lean_sweep_with_a_given_upstream(ebos, triple, name):
    """splits 1, 2, 3 and the adaptive work items (0) wherever ``ebos_plan_parts`` cuts a tile -- every set but a, by the model of
    the case file, which the plan's part table must agree with."""
    from event_based_bos_amd import event_plan as EP

    tile, halo = triple[:2], triple[2]
    size, tile = B.geometry_of(tile)
    ev, fl, up = B.window(tile, name), B.flow(size), B.upstream(size)
    plan = plan_of(ebos, name, ev, size, tile, "compact")
    assert plan.lean and plan.compact and plan.n == len(ev) and plan.dt_bound == 1.0
    want = general_grad(ebos, (name, "plain"), ev, size, tile, fl, up)
    n_cu = EP._n_cu(plan.device)
    parts = parts_of(plan)
    assert parts == B.adaptive_parts(SETS[name], n_cu, EP.part_fixed_events(plan.n, 4, n_cu)), (parts, n_cu)
    assert (max(parts) > 1) == (name != "a") or n_cu != B.N_CU_MODEL, parts
    flow, upg = G(fl, torch.float32), G(up, torch.float32)
    for splits in (1, 2, 3, 0):
        if splits == 0 and max(parts) == 1:
            print(f"[{triple} set {name}] ebos_plan_parts cuts no tile of {SETS[name]}: the adaptive work items are the tiles")
            continue
        got, again = grad_up(plan, flow, upg, halo, splits), grad_up(plan, flow, upg, halo, splits)
        assert torch.equal(got, again), splits
        check(f"{triple} set {name} splits {splits}" + (f" parts {parts}" if splits == 0 else ""), got, want, size, tile, ev, 1.0)


@pytest.mark.parametrize("kind", ["speculative", "restaged"])
def test_lean_sweep_with_run_time_windows(ebos, kind):
    """halo="auto" (the DYN instantiation): a field the 4 px speculative window holds, and one with a tile of 20 px for which the
    window is staged again -- the early chunk requests (BwdPre) are decoded after either."""
    size, tile = B.geometry_of(MAIN[:2])
    ev, up = B.window(tile, "e"), B.upstream(size)
    fl = B.flow(size, amp=B.SPEC_FLOW_AMP) if kind == "speculative" else B.reach_flow(size, tile)
    plan = plan_of(ebos, "e", ev, size, tile, "compact")
    want = general_grad(ebos, ("e", "auto-" + kind), ev, size, tile, fl, up)
    flow, upg = G(fl, torch.float32), G(up, torch.float32)
    for splits in (1, 0):
        got, again = grad_up(plan, flow, upg, "auto", splits), grad_up(plan, flow, upg, "auto", splits)
        assert torch.equal(got, again)
        check(f"auto {kind} splits {splits}", got, want, size, tile, ev, 1.0)


# ------------------------------------------------------------------------------------------ 2. cost path
COST = [(t, s, o) for t in (MAIN, (32, 32, 8)) for s in "de" for o in (False, True)]


@pytest.mark.parametrize("triple,name,omit", COST, ids=["x".join(map(str, t)) + "-" + s + ("-omit-pad2" if o else "") for t, s, o in COST])
def test_variance_cost_path(ebos, triple, name, omit):
    tile, halo = triple[:2], triple[2]
    size, tile = B.geometry_of(tile)
    ev, fl = B.window(tile, name), B.flow(size)
    pad = (2, 2) if omit else (0, 0)
    plan = plan_of(ebos, name, ev, size, tile, "compact")
    full = plan_of(ebos, name, ev, size, tile, "full")
    flow = G(fl, torch.float32)
    v, got = grad_cost(plan, flow, halo, omit, pad)
    v2, again = grad_cost(plan, flow, halo, omit, pad)
    v_gen, want = grad_cost(full, flow, None, omit, pad)
    v_ref, g_ref = B.ref_variance_grad((name, tile), ev, fl, size, omit, pad)
    e_gen, e_ref = rel(got.cpu().numpy(), want.cpu().numpy()), rel(got.cpu().numpy(), g_ref)
    print(f"[cost {triple} set {name} omit {omit} pad {pad}] variance {v!r} (general {v_gen!r}, f64 {v_ref!r}); gradient rel-L2 against the "
          f"general kernels {e_gen:.2e}, against the f64 oracle {e_ref:.2e}")
    assert torch.equal(got, again) and v == v2
    assert abs(v - v_ref) <= 1e-5 * abs(v_ref)
    assert e_gen < BAR_GENERAL and e_ref < BAR_ORACLE


# ------------------------------------------------------------------------------------------ 3. spill sweep on a large work item
@pytest.mark.parametrize("triple", [MAIN, (32, 32, 8)], ids=lambda t: "x".join(map(str, t)))
def test_spill_sweep_draws_its_chunks_afresh(ebos, triple):
    """A row of 40 px through the 24 577-event tile: the events that leave the window sit in chunks >= 32 of the plan (asserted by the
    CPU test of the cases), which the second sweep only sees if the queue was reset in front of it."""
    tile, halo = triple[:2], triple[2]
    size, tile = B.geometry_of(tile)
    ev, fl, up = B.window(tile, "e"), B.row_flow(size, tile), B.upstream(size)
    n_out = int(B.beyond_window(ev, fl, size, tile, halo).sum())
    assert n_out > 0
    plan = plan_of(ebos, "e", ev, size, tile, "compact")
    want = general_grad(ebos, ("e", "row"), ev, size, tile, fl, up)
    flow, upg = G(fl, torch.float32), G(up, torch.float32)
    for splits in (1, 0):
        got, again = grad_up(plan, flow, upg, halo, splits), grad_up(plan, flow, upg, halo, splits)
        assert torch.equal(got, again)   # (the spill sweep's run sums are integer adds into the same LDS words)
        check(f"spill {triple} ({n_out} events beyond the window) splits {splits}", got, want, size, tile, ev, 1.0)
    # the row's own pixels, on their own: the gradient of the events the second sweep handles
    r = B.spill_row(size, tile)
    rs, cs = B.tile_slices(size, tile)[3]
    e_row = rel(got.cpu().numpy()[:, r, cs], want[:, r, cs])
    print(f"[spill {triple}] row {r} of tile 3 alone: rel-L2 {e_row:.2e}")
    assert e_row < BAR_GENERAL


# ------------------------------------------------------------------------------------------ 4. f64 redo after *bad
@pytest.mark.parametrize("name", ["d", "e"])
def test_f64_redo_of_a_before_plan(ebos, name):
    """Reference time "before": dt in [1, 2].  The fixed-point main sweep checks |dt| on the events against the bound it was given
    and raises *bad where they exceed it -- the variance job of the existing test hands it none and assumes 1 --; the slice is then
    redone in f64, drawing its chunks afresh.  Either way: the gradient of the general kernels, from every chunk."""
    size, tile = B.geometry_of(MAIN[:2])
    ev, fl, up = B.window(tile, name), B.flow(size), B.upstream(size)
    plan = plan_of(ebos, name, ev, size, tile, "compact", "before")
    assert plan.dt_bound == 2.0
    want = general_grad(ebos, (name, "plain"), ev, size, tile, fl, up, "before")
    flow, upg = G(fl, torch.float32), G(up, torch.float32)
    for halo in (32, "auto"):
        check(f"before set {name} halo {halo}", grad_up(plan, flow, upg, halo, 1), want, size, tile, ev, 1.0, 2.0)
    full = plan_of(ebos, name, ev, size, tile, "full", "before")
    for halo in (32, "auto"):   # the trigger of the existing test: the variance job, which passes no bound of the plan's
        _, got = grad_cost(plan, flow, halo)
        _, gen = grad_cost(full, flow, None)
        e = rel(got.cpu().numpy(), gen.cpu().numpy())
        print(f"[before set {name} halo {halo}] variance gradient against the general kernels {e:.2e}")
        assert e < BAR_GENERAL


@pytest.mark.parametrize("name", ["d", "e"])
def test_f64_redo_after_a_spilled_tap_reaches_an_upstream_spike(ebos, name):
    """A 30 px field against halo 8 and an upstream value of 1e6 outside the windows of tiles 1 .. 3: a run sum of their spill sweep
    leaves the range (*bad) and the slice is redone in f64, drawing its chunks afresh; tile 0 stages the spike and takes f64 from
    the start."""
    size, tile = B.geometry_of((32, 32))
    ev, fl, up = B.window(tile, name), B.aimed_flow(size, tile), B.spike_upstream(size, tile)
    plan = plan_of(ebos, name, ev, size, tile, "compact")
    want = general_grad(ebos, (name, "spike"), ev, size, tile, fl, up)
    flow, upg = G(fl, torch.float32), G(up, torch.float32)
    for splits in (1, 0):
        got = grad_up(plan, flow, upg, B.HALO_MIN, splits)
        check(f"spike set {name} splits {splits}", got, want, size, tile, ev, B.SPIKE)
    # away from the source pixels whose events touch the spike the gradient is of the order of 1, and the image norm (1e6) would
    # hide the loss of all of it: those pixels on their own
    hit = B.touches(ev, fl, B.spike_pixel(tile))
    quiet = np.ones(size, dtype=bool)
    quiet[ev[hit, 0].astype(int), ev[hit, 1].astype(int)] = False
    e_quiet = rel(got.cpu().numpy()[:, quiet], want[:, quiet])
    print(f"[spike set {name}] {int(hit.sum())} events touch the spike; the {int(quiet.sum())} source pixels that do not: rel-L2 {e_quiet:.2e}")
    assert e_quiet < BAR_GENERAL


# ------------------------------------------------------------------------------------------ 5. hot-pixel tile
def test_hot_pixel_tile_takes_f64_from_the_start(ebos):
    size, tile = B.geometry_of(MAIN[:2])
    ev, fl, up = B.window(tile, "e", hot=B.HOT), B.flow(size), B.upstream(size)
    plan = plan_of(ebos, "e-hot", ev, size, tile, "compact")
    want = general_grad(ebos, ("e-hot", "plain"), ev, size, tile, fl, up)
    flow, upg = G(fl, torch.float32), G(up, torch.float32)
    got, again = grad_up(plan, flow, upg, 32, 1), grad_up(plan, flow, upg, 32, 1)
    check("hot pixel", got, want, size, tile, ev, 1.0)
    for k, (rs, cs) in enumerate(B.tile_slices(size, tile)[:3]):   # the other tiles stay fixed point
        assert torch.equal(got[:, rs, cs], again[:, rs, cs]), k
    rs, cs = B.tile_slices(size, tile)[3]
    e_hot = rel(got.cpu().numpy()[:, rs, cs], want[:, rs, cs])
    print(f"[hot pixel] tile 3 alone rel-L2 {e_hot:.2e}; repeat bit for bit there: {torch.equal(got[:, rs, cs], again[:, rs, cs])}")
    assert e_hot < BAR_GENERAL


# ------------------------------------------------------------------------------------------ 6. loops of plans that are not lean
NONLEAN = [(s, k) for s in "fg" for k in ("weights", "xydt", "xydt-weights")]


@pytest.mark.parametrize("name,kind", NONLEAN, ids=[f"{s}-{k}" for s, k in NONLEAN])
def test_static_stride_loop_of_plans_that_are_not_lean(ebos, name, kind):
    """1023, 1024, 1025, 2048 and 2049 groups in a tile, around the kBlock stride of the general tile loop (per-event weights on the
    compact format, the (x, y, dt) format of fractional source coordinates, both)."""
    size, tile = B.geometry_of(MAIN[:2])
    frac, weighted = kind.startswith("xydt"), kind.endswith("weights")
    ev, fl, up = B.window(tile, name, fractional=frac), B.flow(size), B.upstream(size)
    plan = plan_of(ebos, name + ("-frac" if frac else ""), ev, size, tile, "full")
    assert plan.compact != frac and not plan.lean and plan.n == len(ev)
    flow, upg = G(fl, torch.float32), G(up, torch.float32)
    w_np = B.weights(len(ev)) if weighted else None
    w = None if w_np is None else G(w_np, torch.float32)
    got, want = grad_up(plan, flow, upg, 32, 1, w), grad_up(plan, flow, upg, None, 1, w)
    if weighted:
        (got, got_w), (want, want_w) = got, want
        e_w = rel(got_w.cpu().numpy(), want_w.cpu().numpy())
        print(f"[{name} {kind}] d_weight against the general kernels {e_w:.2e}")
        assert e_w < BAR_GENERAL and torch.count_nonzero(want_w).item() > 0.9 * len(ev)
    check(f"{name} {kind}", got, want.cpu().numpy(), size, tile, ev, 1.0 if not weighted else 1.5)
    ref = B.ref_upstream_grad((name, kind), ev, fl, up, size, w_np)
    e_ref = rel(got.cpu().numpy(), ref)
    print(f"[{name} {kind}] against the f64 oracle{' (weight=)' if weighted else ''} {e_ref:.2e}")
    assert e_ref < BAR_ORACLE


# ------------------------------------------------------------------------------------------ 7. forward redo past 32 chunks
def both_forward_routes(plan, flow):
    built, again = plan.iwe_dense(flow, halo=32, splits=1), plan.iwe_dense(flow, halo=32, splits=1)
    auto = plan.iwe_dense(flow, halo="auto", splits=1)
    return built, again, auto


def test_forward_redo_of_a_hot_pixel_past_32_chunks(ebos):
    """The hot-pixel wrap of tests/test_dense_loop_two_groups.py on set e: the exact redo of the 24 577-event tile must draw chunks
    32 .. 96 afresh."""
    size, tile = B.geometry_of(MAIN[:2])
    ev = B.window(tile, "e", hot=B.HOT_WRAP)
    plan = plan_of(ebos, "e-wrap", ev, size, tile, "compact")
    built, again, auto = both_forward_routes(plan, G(np.zeros((2,) + size), torch.float32))
    counts = B.pixel_counts(ev, size)
    print(f"[forward hot pixel] max {built.max().item()}, sum {built.sum().item()} of {len(ev)}, built == auto {torch.equal(built, auto)}")
    assert np.array_equal(built.cpu().numpy(), counts.astype(np.float32))       # zero flow: the event histogram, exact
    assert torch.equal(built, auto) and torch.equal(built, again)


def test_forward_redo_of_a_nan_flow_past_32_chunks(ebos):
    size, tile = B.geometry_of(MAIN[:2])
    ev, fl = B.window(tile, "e"), B.flow(size).copy()
    i = int(np.nonzero(B.tile_index(ev, size, tile) == 3)[0][7])
    r, c = int(ev[i, 0]), int(ev[i, 1])
    on_pixel = (ev[:, 0] == r) & (ev[:, 1] == c)
    fl[0, r, c] = np.nan
    plan = plan_of(ebos, "e", ev, size, tile, "compact")
    built, again, auto = both_forward_routes(plan, G(fl, torch.float32))
    clean = fl.copy()
    clean[0, r, c] = 0.0
    want = O.iwe_dense(torch.from_numpy(ev[~on_pixel]), torch.from_numpy(clean), size).numpy()
    err = rel(built.cpu().numpy(), want)
    print(f"[forward NaN flow at ({r}, {c}), {int(on_pixel.sum())} events] built == auto {torch.equal(built, auto)}, oracle rel-L2 {err:.2e}")
    assert torch.isfinite(built).all() and on_pixel.sum() >= 1
    assert torch.equal(built, auto) and torch.equal(built, again)
    assert err < 1e-5


# ------------------------------------------------------------------------------------------ 8. GRID backward, resident kernel
def test_grid_backward_and_resident_kernel_on_set_e(ebos):
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    size, tile = B.geometry_of(MAIN[:2])
    ev = B.window(tile, "e")
    plan = plan_of(ebos, "e", ev, size, tile, "full")
    assert plan.compact
    patch = (24, 32)
    gh, gw = O.patch_grid_shape(size, patch, patch)
    theta0 = torch.from_numpy(np.random.RandomState(3).uniform(-2, 2, (2, gh, gw))).float()

    def make(sample_grid=None):
        return FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.01, 0.02, halo="auto", lr=0.1, capacity=4, splits=1, sample_grid=sample_grid)

    grid, dense = make(), make(False)
    assert grid.sample_grid and not dense.sample_grid
    l_g, g_g = grid.value_and_grad(theta0.cuda())
    l_d, g_d = dense.value_and_grad(theta0.cuda())
    e_loss, e_grad = abs(float(l_g) / float(l_d) - 1), float((g_g - g_d).norm() / g_d.norm())
    t64 = theta0.double().requires_grad_(True)
    field = O.upsample_patch_flow(t64, size, patch, patch)
    loss = O.image_variance(O.iwe_dense(torch.from_numpy(ev), field, size)) + 0.01 * O.flow_norm(field)
    loss = loss + 0.02 * O.image_gradient_tv(field, torch.ones(size, dtype=torch.float64))
    loss.backward()
    o_loss, o_grad = abs(float(l_g) - loss.item()) / abs(loss.item()), rel(g_g.cpu().numpy(), t64.grad.numpy())
    print(f"[grid route] against the dense route: loss rel {e_loss:.2e}, d_theta rel-L2 {e_grad:.2e}; against the f64 oracle: loss rel "
          f"{o_loss:.2e}, d_theta rel-L2 {o_grad:.2e}")
    assert e_loss < 1e-6 and e_grad < 1e-5
    assert o_loss <= 1e-5 and o_grad < BAR_ORACLE
    pipe, res = make(), make()
    want = pipe.run(3, resident=False).cpu().numpy()
    assert pipe.last_run_mode == "pipeline"
    if res.resident_supported():
        got = res.run(3, resident=True).cpu().numpy()
        print(f"[resident] mode {res.last_run_mode}, status {res.resident_status}, losses {got} / pipeline {want}")
        if res.last_run_mode != "resident":
            # the launch itself declined the window (-101 a wait passed its cap, -102 a tap left the largest window, -104 a crowded
            # tile): the pipeline ran the iterations it left
            assert res.resident_status in (-101, -102, -104) and res.last_run_mode in ("pipeline", "resident+pipeline")
    else:
        why = (ebos.load_library().ebos_last_error() or b"").decode()
        print(f"[resident] not supported for this window: {why}")
        assert why
        got = res.run(3).cpu().numpy()
        assert res.last_run_mode == "pipeline"
    np.testing.assert_array_equal(got, want)
    assert res.t == 3 and torch.equal(res.theta, pipe.theta)


# ------------------------------------------------------------------------------------------ 9. persistent batch
def test_persistent_batch_over_windows_that_cross_the_queue_threshold(ebos):
    """SlabBatch: one tile goes 0 -> 8193 -> 1 -> 24577 -> 0 events from window to window; a window's first chunks are requested
    while the previous window is still being stored.  Every image is the per-plan image, bit for bit."""
    size, tile = B.geometry_of(MAIN[:2])
    windows = B.batch_windows(tile)
    plans = [plan_of(ebos, f"batch{k}", ev, size, tile, "compact") for k, ev in enumerate(windows)]
    flows = [G(B.flow(size, seed=40 + k), torch.float32) for k in range(len(windows))]
    for halo in (32, 16):
        batch = ebos.SlabBatch(plans, flows, halo=halo, splits=1)
        var = batch.run().cpu().numpy()
        for k, (pl, fl) in enumerate(zip(plans, flows)):
            single = pl.iwe_dense(fl, halo=halo, splits=1)
            assert torch.equal(batch.iwes[k], single), (halo, k)
        again = batch.run().cpu().numpy()
        assert np.array_equal(var, again)
        errs = [rel(batch.iwes[k].cpu().numpy(), O.iwe_dense(torch.from_numpy(windows[k]), torch.from_numpy(B.flow(size, seed=40 + k)),
                                                             size).numpy()) for k in (1, 3)]
        print(f"[batch halo {halo}] variances {var}; windows 1 and 3 against the f64 oracle {errs[0]:.2e}, {errs[1]:.2e}")
        assert max(errs) < 1e-5
