"""GPU tests of the time-aware kernels (csrc/warp_voxel.hip, warp_voxel_multiref.hip, warp_voxel_core.h and the loops of cmax_voxel.hip
over them) on EVERY built (tile_h, tile_w, halo), on runs of chosen lengths and with more than 64 bins.  The sibling files run one
geometry -- 37 x 70, plan tile (32, 32), T = 5 or a T = 255 with eight events to a pixel --; here the windows of
tests/_voxel_tile_cases.py (pinned on the CPU by tests/test_voxel_tile_cases.py) give every tile shape interior tiles, four-window
corners, overhang on both axes, whole empty tiles, events beyond every halo, and the pixel-owner backward runs of exactly 1 .. 129 and
300 events whose bins fill every register slot of its whole-wave walk.

Yardsticks: CPU, float64, torch autograd (tests/_warp_voxel_ref.py and what tests/_voxel_tile_cases.py composes of it).  Bars are the
project's (tests/test_gpu_warp_voxel.py, tests/test_gpu_voxel_loop.py): IWE relative L2 < 1e-4 -- relative to the image's norm but not
below 0.05, the floor of tests/test_gpu_parity.py::test_fuzz_fused_path_against_oracle, where a flow pushes most of the mass out of the
image --, contrast value relative < 1e-5, gradients relative L2 < 1e-3.  On the constructed runs the gradient bar also holds for EACH
constructed pixel's own [T, 2] column against that column of the yardstick, and its cells are exactly 0.0 in the bins the pixel holds no
event of: a sum kept in the wrong lane or register slot lands in another bin and fails alone, where the whole-field L2 would not move.

Measured on an MI355X (DESIGN 4.28 has the tables): every triple IWE 4.4e-7 - 5.7e-7, through the spill path at most 4.9e-6 (the
(64, 64, 64) window at +-160 px, K references with |dt| up to 2); values at most 1.3e-7; d_voxel and d_theta at most 1.9e-6; the worst
constructed pixel against its own column 1.6e-5 (a run of 7 at T = 64), the same on every tile shape and in the single, batch and
K-reference kernels.  Every test prints what the kernels give, one ``VT|`` line per comparison."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxel_launch as K  # noqa: E402
import _voxel_tile_cases as V  # noqa: E402
from _voxel_tile_cases import BMA, CONSTRUCTED, DIRECTIONS, G, MAIN, PATCH, PLAN_TILES, T5, TINY, rel  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = torch.float32
IWE_BAR, VALUE_BAR, GRAD_BAR, NORM_FLOOR = 1e-4, 1e-5, 1e-3, 0.05
# (plan tile, T) of the owner backward on the runs window: every tile shape at T = 5 and 255; 64 | 65 (one register slot | two) and 129
# (three) on the square tile and on the one whose rows are the shortest
OWNER_CASES = [(t, T) for t in PLAN_TILES for T in (T5, 255)] + [(t, T) for t in ((32, 32), (16, 64)) for T in (64, 65, 129)]
ONE_PER_SHAPE = tuple((th, tw, 32) for th, tw in PLAN_TILES)
LOOP_TILES = ((64, 64), (32, 64), (16, 64))


def built_triples():
    """The library's own table where it is there to ask (collection must not need it), else the nine it is known to hold."""
    from event_based_bos_amd import _hip

    if os.path.exists(os.environ.get("EBOS_HIP_LIBRARY", _hip.LIB_PATH)):
        return tuple(_hip.tiled_configs())
    return V.BUILT


def tid(t):
    return "x".join(str(int(a)) for a in t) if isinstance(t, tuple) else str(t)


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


@pytest.fixture(scope="module")
def lib(ebos):
    from event_based_bos_amd import _hip

    return _hip.require_gpu()


_plans = {}


def plan_of(ebos, name, ev, tile, T=T5, shape=MAIN):
    """One plan per (window name, tile, T) for the module (``tile=None``: un-binned)."""
    key = (name, tile, T, tuple(shape))
    if key not in _plans:
        _plans[key] = ebos.EventPlan.build(G(ev), shape, "first", True, tile=tile, emit="full", time_bin=T)
    return _plans[key]


def iwe_err(got, want):
    got = got.detach().cpu().double().numpy()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), NORM_FLOOR))


def check_iwe(tag, got, want):
    err = iwe_err(got, want)
    print(f"VT|iwe|{tag}|{err:.3e}|mass {float(got.sum()):.1f}")
    assert bool(torch.isfinite(got).all()), tag
    assert tuple(got.shape) == tuple(want.shape) and err < IWE_BAR, (tag, err)


def check_value(tag, got, want):
    err = abs(float(got.detach()) - want) / abs(want)
    print(f"VT|value|{tag}|{err:.3e}")
    assert err < VALUE_BAR, (tag, err)


def check_grad(tag, got, want, runs=None):
    """Finite, whole field within the bar; with ``runs`` = (events, T) of a runs window: every constructed pixel's column within the bar
    on its own, and exactly 0.0 in the bins it holds no event of."""
    assert bool(torch.isfinite(got).all()), tag
    whole = rel(got, want)
    print(f"VT|grad|{tag}|{whole:.3e}")
    assert tuple(got.shape) == tuple(want.shape) and whole < GRAD_BAR, (tag, whole)
    if runs is not None:
        ev, T = runs
        cols = {p: V.column_rel(got, want, p) for p in CONSTRUCTED}
        worst = max(cols, key=cols.get)
        print(f"VT|pixel|{tag}|{cols[worst]:.3e}|worst pixel {worst} of run {CONSTRUCTED[worst]}")
        assert cols[worst] < GRAD_BAR, (tag, cols)
        check_empty_bins(tag, got, ev, T)


def check_empty_bins(tag, got, ev, T):
    mask = torch.from_numpy(V.empty_bins_mask(ev, T)).to(got.device)
    assert int(torch.count_nonzero(got[:, 0][mask])) == 0 and int(torch.count_nonzero(got[:, 1][mask])) == 0, tag


def fixed_upstream(lead, pad, shape=MAIN, seed=7):
    """(g_images lead + [h, w], affine lead + [2]): an upstream that does not come from a forward, whose float atomics differ between runs."""
    rs = np.random.RandomState(seed)
    return (G(rs.uniform(-1, 1, tuple(lead) + (shape[0] + 2 * pad, shape[1] + 2 * pad)), F32), G(rs.uniform(0.5, 2, tuple(lead) + (2,)), F32))


def batch_stack(ebos, tile, T=T5):
    """(plans [p0, None, p2], their stack, voxels [3, T, 2, H, W] f32) of ``V.batch_windows(T)``: window 1 holds no events."""
    w = V.batch_windows(T)
    plans = [plan_of(ebos, "runs", w[0], tile, T), None, plan_of(ebos, "batch2", w[2], tile, T)]
    return plans, K.StackWithEmpty(ebos, plans), G(np.stack(V.batch_voxels(T)), F32).contiguous()


# ---------------------------------------------------------------------------------------------- a. every built triple, forward
def test_the_sweep_is_the_built_set(ebos):
    from event_based_bos_amd import _hip

    assert set(built_triples()) == set(_hip.tiled_configs()) == set(V.BUILT) and len(_hip.tiled_configs()) == 9
    assert {t[:2] for t in V.BUILT} == set(PLAN_TILES) and set(ONE_PER_SHAPE) <= set(V.BUILT)


@pytest.mark.parametrize("triple", built_triples(), ids=tid)
def test_forward_single_entry(ebos, triple):
    from event_based_bos_amd.event_plan import _voxel_halo

    th, tw, hl = triple
    ev, vx = V.main_window(), V.voxel_u(MAIN)
    plan = plan_of(ebos, "main", ev, (th, tw))
    assert _voxel_halo(plan, hl) == hl                             # the tiled entry, not the general kernel
    vox, w = G(vx, F32), G(V.weights_of(len(ev)), F32)
    for pad in (0, 2):
        for splits in (1, 3):
            for weighted in (False, True):
                got = plan.iwe_voxel(vox, pad=(pad, pad), weight=w if weighted else None, halo=hl, splits=splits)   # (raises unless OK)
                check_iwe(f"a-single {tid(triple)} pad {pad} splits {splits} weighted {weighted}", got, V.ref_iwe("main", ev, vx, pad, weighted))


@pytest.mark.parametrize("triple", built_triples(), ids=tid)
def test_value_and_gradient_behind_every_triple(ebos, triple):
    """The contrast and its three backwards (pixel-owner for one and for K = 3 reference times, atomic) behind the forward of every
    triple on the main window: the value is the forward's, the backwards take the tile at run time."""
    th, tw, hl = triple
    ev, vx = V.main_window(), V.voxel_u(MAIN)
    plan = plan_of(ebos, "main", ev, (th, tw))
    vox = G(vx, F32)
    tag = f"a-contrast {tid(triple)}"
    var_ref, dv_ref = V.ref_variance_grad("main", ev, vx, True, 2)
    out = K.all_ones((T5, 2) + MAIN)
    value, _ = plan.variance_voxel_value_and_grad(vox, True, pad=(2, 2), halo=hl, out=out)
    check_value(tag + " owner", value, var_ref)
    check_grad(tag + " owner", out, dv_ref)
    v = vox.clone().requires_grad_(True)
    value = plan.contrast_voxel(v, "image_variance", True, pad=(2, 2), halo=hl, splits=3)
    value.backward()
    check_value(tag + " atomic", value, var_ref)
    check_grad(tag + " atomic", v.grad, dv_ref)
    varK_ref, dvK_ref = V.ref_mean_variance_grad("main", ev, vx, DIRECTIONS[3])
    outK = K.all_ones((T5, 2) + MAIN)
    valueK, _ = plan.variance_voxel_multi_value_and_grad(vox, list(DIRECTIONS[3]), halo=hl, out=outK)
    check_value(tag + " owner K3", valueK, varK_ref)
    check_grad(tag + " owner K3", outK, dvK_ref)


@pytest.mark.parametrize("triple", built_triples(), ids=tid)
def test_forward_batch_entry(ebos, lib, triple):
    th, tw, hl = triple
    windows, voxels = V.batch_windows(), V.batch_voxels()
    _, stack, vox = batch_stack(ebos, (th, tw))
    for pad, splits in ((0, 1), (2, 3)):
        buf, iwe = K.guarded(shape=(3, MAIN[0] + 2 * pad, MAIN[1] + 2 * pad))
        iwe.zero_()                                                # (the entry point accumulates)
        K.tiled_batch(lib, stack, vox, hl, iwe, pad=pad, splits=splits, shape=MAIN)
        torch.cuda.synchronize()
        assert K.guards_untouched(buf) and int(torch.count_nonzero(iwe[1])) == 0
        for b in (0, 2):
            check_iwe(f"a-batch {tid(triple)} pad {pad} splits {splits} window {b}", iwe[b], V.ref_iwe(("batch", b), windows[b], voxels[b], pad))


@pytest.mark.parametrize("n_ref,pad,splits", [(1, 0, 1), (3, 2, 2), (4, 0, 3)])
@pytest.mark.parametrize("triple", built_triples(), ids=tid)
def test_forward_k_reference_batch_entry(ebos, lib, triple, n_ref, pad, splits):
    th, tw, hl = triple
    directions = DIRECTIONS[n_ref]
    windows, voxels = V.batch_windows(), V.batch_voxels()
    plans, stack, vox = batch_stack(ebos, (th, tw))
    iwes = K.forward_batch(lib, stack, plans[0], vox, directions, hl, pad, splits, shape=MAIN)
    assert iwes.shape == (3, n_ref, MAIN[0] + 2 * pad, MAIN[1] + 2 * pad) and int(torch.count_nonzero(iwes[1])) == 0
    for b in (0, 2):
        want = V.ref_iwes(("batch", b), windows[b], voxels[b], directions, pad)
        for k, d in enumerate(directions):
            check_iwe(f"a-kref {tid(triple)} K {n_ref} window {b} reference {d}", iwes[b, k], want[k])
    # the operator on one window is the same kernel with B = 1
    got = plans[0].iwe_voxel_multi(vox[0], list(directions), pad=(pad, pad), halo=hl, splits=splits)
    want = V.ref_iwes(("batch", 0), windows[0], voxels[0], directions, pad)
    assert max(iwe_err(got[k], want[k]) for k in range(n_ref)) < IWE_BAR


# ---------------------------------------------------------------------------------------------- b. events beyond the halo
@pytest.mark.parametrize("triple", built_triples(), ids=tid)
def test_events_beyond_the_halo(ebos, lib, triple):
    th, tw, hl = triple
    amp = V.SPILL_AMP[triple]
    ev, vx = V.spill_window(amp), V.voxel_u(MAIN, T5, amp)
    beyond = V.events_beyond(ev, vx, triple)
    print(f"VT|beyond|b {tid(triple)} amp {amp}|{beyond} of {len(ev)} events beyond the halo, inside the image")
    assert beyond >= V.SPILL_MIN
    plan = plan_of(ebos, ("spill", amp), ev, (th, tw))
    vox = G(vx, F32)
    for pad, splits in ((0, 1), (2, 3)):
        got = plan.iwe_voxel(vox, pad=(pad, pad), halo=hl, splits=splits)
        check_iwe(f"b-single {tid(triple)} amp {amp} pad {pad} splits {splits}", got, V.ref_iwe(("spill", amp), ev, vx, pad))
    # K references whose |dt| reaches 2
    sh = K.c_shifts(plan, BMA)[0]
    assert float((plan.dt[:plan.n] + sh[2]).min()) < -1.9 and float((plan.dt[:plan.n] + sh[0]).max()) > 1.9
    print(f"VT|beyond|b {tid(triple)} amp {amp}|before / middle / after: {[V.events_beyond(ev, vx, triple, d) for d in BMA]}")
    iwes = K.forward(lib, plan, vox, BMA, hl, 0, splits=2, shape=MAIN)
    want = V.ref_iwes(("spill", amp), ev, vx, BMA, 0)
    for k, d in enumerate(BMA):
        check_iwe(f"b-kref {tid(triple)} amp {amp} reference {d}", iwes[k], want[k])


# ---------------------------------------------------------------------------------------------- c. owner backward on constructed runs
@pytest.mark.parametrize("tile,T", OWNER_CASES, ids=tid)
def test_owner_backward_single(ebos, lib, tile, T):
    ev, vx = V.runs_window(T), V.voxel_u(MAIN, T)
    var_ref, dv_ref = V.ref_variance_grad(("runs", T), ev, vx)
    plan = plan_of(ebos, "runs", ev, tile, T)
    vox = G(vx, F32)
    out = K.all_ones((T, 2) + MAIN)
    value, d_voxel = plan.variance_voxel_value_and_grad(vox, out=out)
    assert d_voxel.data_ptr() == out.data_ptr()
    tag = f"c-single tile {tid(tile)} T {T}"
    check_value(tag, value, var_ref)
    check_grad(tag, out, dv_ref, (ev, T))
    g_image, affine = fixed_upstream((), 0)
    a, b = (K.owner_single(lib, plan, vox, g_image, affine, 0, 0, shape=MAIN) for _ in range(2))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and int(torch.count_nonzero(a)) > 0
    check_empty_bins(tag, a, ev, T)


@pytest.mark.parametrize("n_ref", [3, 4])
@pytest.mark.parametrize("tile,T", OWNER_CASES, ids=tid)
def test_owner_backward_k_references(ebos, lib, tile, T, n_ref):
    directions = DIRECTIONS[n_ref]
    ev, vx = V.runs_window(T), V.voxel_u(MAIN, T)
    var_ref, dv_ref = V.ref_mean_variance_grad(("runs", T), ev, vx, directions)
    plan = plan_of(ebos, "runs", ev, tile, T)
    vox = G(vx, F32)
    out = K.all_ones((T, 2) + MAIN)
    value, d_voxel = plan.variance_voxel_multi_value_and_grad(vox, list(directions), out=out)
    assert d_voxel.data_ptr() == out.data_ptr()
    tag = f"c-kref{n_ref} tile {tid(tile)} T {T}"
    check_value(tag, value, var_ref)
    check_grad(tag, out, dv_ref, (ev, T))
    g_images, affine = fixed_upstream((n_ref,), 0)
    a, b = (K.owner_backward(lib, plan, vox, directions, g_images, affine, 0, 0, shape=MAIN) for _ in range(2))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and int(torch.count_nonzero(a)) > 0
    check_empty_bins(tag, a, ev, T)


@pytest.mark.parametrize("tile,T", OWNER_CASES, ids=tid)
def test_owner_backward_batch(ebos, lib, tile, T):
    from event_based_bos_amd.event_plan import _image_variances, _variance_affines

    windows, voxels = V.batch_windows(T), V.batch_voxels(T)
    _, stack, vox = batch_stack(ebos, tile, T)
    iwe = torch.zeros((3,) + MAIN, dtype=F32, device=V.dev())
    K.tiled_batch(lib, stack, vox, 32, iwe, T=T, shape=MAIN)
    values, moments = _image_variances(iwe, False)
    affine = _variance_affines(moments, torch.ones(3, dtype=F32, device=V.dev()))
    outs = []
    for _ in range(2):
        d_voxel = K.all_ones((3, T, 2) + MAIN)
        K.owner_batch(lib, stack, vox, iwe, affine, T, 0, 0, d_voxel, shape=MAIN)
        outs.append(d_voxel)
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    assert int(torch.count_nonzero(outs[0][1])) == 0 and int(torch.count_nonzero(iwe[1])) == 0      # the window of no events
    for b in (0, 2):
        var_ref, dv_ref = V.ref_variance_grad(("runs", T) if b == 0 else ("batch2", T), windows[b], voxels[b])
        tag = f"c-batch tile {tid(tile)} T {T} window {b}"
        check_value(tag, values[b], var_ref)
        check_grad(tag, outs[0][b], dv_ref, (windows[b], T) if b == 0 else None)


# ---------------------------------------------------------------------------------------------- d. atomic backward on the same windows
@pytest.mark.parametrize("T", [T5, 255])
@pytest.mark.parametrize("tile", [(32, 32), (16, 64), None], ids=tid)      # None: an un-binned plan, iwe_voxel_bwd_kernel<false>
def test_atomic_backward_on_constructed_runs(ebos, tile, T):
    ev, vx = V.runs_window(T), V.voxel_u(MAIN, T)
    var_ref, dv_ref = V.ref_variance_grad(("runs", T), ev, vx)
    plan = plan_of(ebos, "runs", ev, tile, T)
    assert plan.binned == (tile is not None)
    v = G(vx, F32).requires_grad_(True)
    value = plan.contrast_voxel(v)
    value.backward()
    tag = f"d-atomic tile {tid(tile)} T {T}"
    check_value(tag, value, var_ref)
    check_grad(tag, v.grad, dv_ref, (ev, T))


# ---------------------------------------------------------------------------------------------- e. empty tiles and the tiny window
@pytest.mark.parametrize("window", ["empty", "tiny"])
@pytest.mark.parametrize("triple", ONE_PER_SHAPE, ids=tid)
def test_empty_tiles_and_a_window_smaller_than_a_tile(ebos, triple, window):
    th, tw, hl = triple
    shape = MAIN if window == "empty" else TINY
    ev, vx = (V.empty_tiles_window() if window == "empty" else V.main_window(TINY)), V.voxel_u(shape)
    plan = plan_of(ebos, window, ev, (th, tw), T5, shape)
    vox = G(vx, F32)
    tag = f"e-{window} {tid(triple)}"
    for pad in (0, 2):
        check_iwe(f"{tag} pad {pad}", plan.iwe_voxel(vox, pad=(pad, pad), halo=hl), V.ref_iwe(window, ev, vx, pad))
    var_ref, dv_ref = V.ref_variance_grad(window, ev, vx)
    out = K.all_ones((T5, 2) + shape)
    value, _ = plan.variance_voxel_value_and_grad(vox, halo=hl, out=out)
    check_value(tag + " owner", value, var_ref)
    check_grad(tag + " owner", out, dv_ref)
    varK_ref, dvK_ref = V.ref_mean_variance_grad(window, ev, vx, DIRECTIONS[3])
    outK = K.all_ones((T5, 2) + shape)
    valueK, _ = plan.variance_voxel_multi_value_and_grad(vox, list(DIRECTIONS[3]), halo=hl, out=outK)
    check_value(tag + " owner K3", valueK, varK_ref)
    check_grad(tag + " owner K3", outK, dvK_ref)
    v = vox.clone().requires_grad_(True)
    value = plan.contrast_voxel(v, halo=hl)
    value.backward()
    check_value(tag + " atomic", value, var_ref)
    check_grad(tag + " atomic", v.grad, dv_ref)
    if window == "empty":                                          # source pixels without events own exact zeros
        for g in (out, outK, v.grad):
            assert int(torch.count_nonzero(g[:, :, 32:, 64:])) == 0


# ---------------------------------------------------------------------------------------------- f. the loops on the other plan tiles
def time_aware(directions=None):
    ta = {"time_bin": T5, "scheme": "upwind", "t0_location": "middle", "clamp": None, "native": True}
    if directions is not None:
        ta["directions"] = list(directions)
    return ta


@pytest.mark.parametrize("owner", [False, True, "K3"])             # K3: three reference times (the owner backward is their only one)
@pytest.mark.parametrize("tile", LOOP_TILES, ids=tid)
def test_loops_on_the_other_plan_tiles(ebos, tile, owner):
    from event_based_bos_amd.solver.time_aware_loop import TimeAwareMultiReferencePatchLoopBatch, TimeAwarePatchLoopBatch

    windows = V.loop_windows()
    directions = V.FML if owner == "K3" else ("first",)
    plans = [plan_of(ebos, ("loop", b), ev, tile) for b, ev in enumerate(windows)]
    theta0 = G(np.stack([V.theta_start(), V.theta_start()]))
    if owner == "K3":
        loop = TimeAwareMultiReferencePatchLoopBatch(plans, PATCH, PATCH, theta0, time_aware(directions), 1.0, lr=0.05, capacity=4)
    else:
        loop = TimeAwarePatchLoopBatch(plans, PATCH, PATCH, theta0, time_aware(), 1.0, lr=0.05, capacity=4, owner_bwd=owner)
    assert loop.halo == 32 and tuple(loop.stack.tile) == tile and loop.owner_bwd == bool(owner)
    start = loop.theta.clone()
    value, grad = loop.value_and_grad(start)
    assert value.shape == (2,) and grad.shape == start.shape and torch.equal(loop.theta, start)
    losses = loop.run(1)
    assert losses.shape == (2, 1) and loop.t == 1 and int(loop.step.item()) == 1
    for b in range(2):
        loss_ref, grad_ref = V.ref_value_and_grad(b, directions)
        tag = f"f-loop tile {tid(tile)} owner {owner} window {b}"
        check_value(tag + " value_and_grad", value[b], loss_ref)
        check_value(tag + " run(1)", losses[b, 0], loss_ref)
        for what, g in (("value_and_grad", grad[b]), ("run(1)", loop.d_theta[b])):
            err = rel(g, grad_ref)
            print(f"VT|grad|{tag} d_theta {what}|{err:.3e}")
            assert bool(torch.isfinite(g).all()) and err < GRAD_BAR, (tag, what, err)
        assert not torch.equal(loop.theta[b], start[b])            # Adam moved every window's grid
