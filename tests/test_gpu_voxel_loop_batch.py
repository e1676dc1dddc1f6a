"""GPU tests of the batched time-aware loop: the batched stages (``ebos_upsample_patch_flow_batch_f32``, ``ebos_flow_regularisers_batch_f32``,
``ebos_iwe_voxel_tiled_batch_f32``, ``ebos_iwe_voxel_owner_bwd_batch_f32``, ``ebos_upsample_patch_flow_bwd[_adam]_batch_f32``), the loop
of one C call for B windows (``TimeAwarePatchLoopBatch``: ``ebos_cmax_voxel_solve_batch_f32``) and ``ContrastMaximization.estimate_batch``.

Shapes: 37 x 70, plan tile (32, 32) with halo 32 -- tiles overhang both axes --, patch (12, 14).  The batch is B = 3 windows that differ
in size, so that a wrong window index shows: w0 a kink-free 20 000-event window, w1 its first event + every third event of the interior
+ its last event (the time range, and so every kept event's bin and warp, is unchanged; a subset of a kink-free window is kink-free),
w2 = ``with_hot_pixel(w0, ...)`` (3 000 more events on one pixel, their bins shuffled).  Voxels, start grids and gradient images differ
per window: w0 is drawn kink-free under all three windows' voxels.

Yardsticks: the single-window entry points (bit for bit, where a stage is deterministic) and the float64 CPU restatements of
tests/_voxel_loop_cases.py.  Bars are the project's: forward images relative L2 < 1e-4, values relative < 1e-5, gradients relative
L2 < 1e-3."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxel_loop_cases as C  # noqa: E402
from _voxel_loop_cases import G, H, N, PATCH, R, T5, W, rel  # noqa: E402
from _voxel_launch import P, S, ok, owner_batch, stack_of, tiled_batch  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3
HALO = 32
# Test 5's tolerance.  How far the SINGLE-window loop (``TimeAwarePatchLoop``, owner backward) lies from the float64 ``torch.optim.Adam``
# loop on each window from that window's start, |loss - loss64| / |loss64| per iteration, measured on an MI355X with the parent's loop
# (never with the batch loop; ``test_five_iterations_follow_the_float64_adam_loop`` prints both on every run):
SINGLE_LOOP_DEVIATION = {
    "w0": (7.48e-08, 5.54e-08, 1.77e-08, 4.42e-08, 2.25e-08),   # 20 000 events, losses -4.38 .. -4.62
    "w1": (4.15e-08, 3.72e-08, 4.66e-08, 1.53e-08, 1.14e-08),   #  6 668 events, losses -1.22 .. -1.28
    "w2": (3.32e-08, 8.41e-08, 2.91e-08, 9.16e-08, 4.86e-08),   # 23 000 events, losses -627 .. -664 (the hot pixel)
}
# (two runs each with the owner and with the atomic backward gave these same figures; so the bounds are 1.50e-7, 9.32e-8 and 1.83e-7.
# In the measured run the batch loop's fifteen losses were the single loops' bit for bit.)
# The batch loop runs the same float32 kernels with the flushes of the forward's tiles in another order: it is allowed twice the largest
# of the window's five figures, the rule of tests/test_gpu_voxel_loop.py.
BATCH_LOOP_FACTOR = 2.0


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


def guarded(shape, dtype=torch.float32, fill=float("nan"), guard=4096):
    """(whole buffer, the view of ``shape`` in its middle): an output with ``guard`` cells in front and behind, all of it ``fill``."""
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), fill, dtype=dtype, device=C.dev())
    return buf, buf[guard:guard + n].view(*shape)


def guards_untouched(buf, guard=4096):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())


# ---------------------------------------------------------------------------------------------- the windows
def off_the_kinks_all(voxels, seed):
    """``C.off_the_kinks`` under SEVERAL voxels at once: N events whose float64-warped coordinates keep 5e-4 px from every integer
    under each of ``voxels`` (a window of the batch is warped by its own voxel; its subsets and supersets keep these events)."""
    margin = 5e-4
    pool = C.O.synth_events(N + 400, H, W, seed=seed, tmin=0.0, tmax=1.0)
    pool[:, 0] += np.random.RandomState(seed + 1).uniform(0, 0.99, len(pool)) * (np.arange(len(pool)) % 2 == 0)
    pool[0, 2], pool[-1, 2] = 0.0, 1.0
    near = np.zeros(len(pool), dtype=bool)
    for vx in voxels:
        warped = R.warp_voxel(torch.from_numpy(pool), torch.from_numpy(np.ascontiguousarray(vx)), "first", True)[0].numpy()
        near |= (np.abs(warped[:, :2] - np.rint(warped[:, :2])) < margin).any(1) & (warped[:, 2] != 0.0)
    near[0] = near[-1] = False                         # (the window is [0, 1] whichever events stay, so every event's warp is fixed)
    ev = np.concatenate([pool[:1], pool[1:-1][~near[1:-1]][:N - 2], pool[-1:]])
    assert len(ev) == N
    return ev


def three_windows(voxels, seed):
    """[w0, w1, w2] for the three voxels ``voxels`` (float64 numpy [T, 2, H, W] each)."""
    w0 = off_the_kinks_all(voxels, seed)
    w1 = np.concatenate([w0[:1], w0[1:-1][::3], w0[-1:]])
    w2 = C.with_hot_pixel(w0, np.ascontiguousarray(voxels[2]))
    assert len(w1) == 2 + len(w0[1:-1][::3]) and len(w2) == N + C.HOT_EXTRA and w1[0, 2] == 0.0 and w1[-1, 2] == 1.0
    return [w0, w1, w2]


def stage_voxels(T=T5):
    return [C.voxel_u(6.0, T, seed=21 + b) for b in range(B)]


def stage_windows():
    """The windows of the stage tests: kink-free under ``stage_voxels()`` (T = 5)."""
    return C.cached("batch_stage_windows", lambda: three_windows(stage_voxels(), seed=41))


# ---------------------------------------------------------------------------------------------- 1. deterministic stages, bit for bit
@pytest.mark.parametrize("shape", [(H, W), (H, 72)])            # scalar stores, and the 16-byte path (W % 4 == 0)
def test_upsample_forward_batch_is_the_single_call(lib, shape):
    h, w = shape
    gh, gw = C.O.patch_grid_shape((h, w), PATCH, PATCH)
    grids = G(np.random.RandomState(3).uniform(-3, 3, (B, 2, gh, gw)), torch.float32)
    outs = []
    for _ in range(2):
        buf, dense = guarded((B, 2, h, w))
        ok(lib.ebos_upsample_patch_flow_batch_f32(P(grids), B, gh, gw, *PATCH, *PATCH, h, w, P(dense), S()), lib)
        assert guards_untouched(buf) and bool(torch.isfinite(dense).all())
        outs.append(dense)
    assert torch.equal(outs[0], outs[1])
    for b in range(B):
        one = torch.empty((2, h, w), dtype=torch.float32, device=C.dev())
        ok(lib.ebos_upsample_patch_flow_f32(P(grids[b]), gh, gw, *PATCH, *PATCH, h, w, P(one), S()), lib)
        assert torch.equal(outs[0][b], one), b
    assert not torch.equal(outs[0][0], outs[0][1])


@pytest.mark.parametrize("shape", [(H, W), (H, 72)])            # scalar stores, and the 16-byte path (W % 4 == 0)
def test_regularisers_batch_is_the_single_call(lib, shape):
    h, w = shape
    n_reg = lib.ebos_flow_regularisers_partials()
    flows = G(np.random.RandomState(5).uniform(-3, 3, (B, 2, h, w)), torch.float32)
    outs = []
    for _ in range(2):
        buf, d_flow = guarded((B, 2, h, w))
        pbuf, partials = guarded((B, n_reg), torch.float64)
        ok(lib.ebos_flow_regularisers_batch_f32(P(flows), B, h, w, 0.1, 0.2, P(d_flow), P(partials), S()), lib)
        assert guards_untouched(buf) and guards_untouched(pbuf) and bool(torch.isfinite(d_flow).all()) and bool(torch.isfinite(partials).all())
        outs.append((d_flow, partials))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for b in range(B):
        d_one = torch.empty((2, h, w), dtype=torch.float32, device=C.dev())
        p_one = torch.empty(n_reg, dtype=torch.float64, device=C.dev())
        ok(lib.ebos_flow_regularisers_f32(P(flows[b]), h, w, 0.1, 0.2, P(d_one), P(p_one), None, 0, 0, None, None, S()), lib)
        assert torch.equal(outs[0][0][b], d_one) and torch.equal(outs[0][1][b], p_one), b
        assert float(p_one.sum()) > 0.0


def owner_inputs(T, pad, seed=7):
    rs = np.random.RandomState(seed)
    voxels = G(np.stack(stage_voxels(T)), torch.float32).contiguous()
    g_images = G(rs.uniform(-1, 1, (B, H + 2 * pad, W + 2 * pad)), torch.float32)
    affine = G(rs.uniform(-1, 1, (B, 2)), torch.float32)
    return voxels, g_images, affine


@pytest.mark.parametrize("T", [1, 5, 255])
@pytest.mark.parametrize("pad,g_lo", [(0, 0), (2, 1)])          # (2, 1): padding and omit_boundary
def test_owner_backward_batch_is_the_single_call(ebos, lib, T, pad, g_lo):
    plans, stack = stack_of(ebos, stage_windows(), T)            # (the bins are made from the events' times for this T)
    voxels, g_images, affine = owner_inputs(T, pad)
    outs = []
    for _ in range(2):
        buf, d_voxel = guarded((B, T, 2, H, W))
        owner_batch(lib, stack, voxels, g_images, affine, T, pad, g_lo, d_voxel)
        assert guards_untouched(buf) and bool(torch.isfinite(d_voxel).all())           # every cell written, nothing beyond
        outs.append(d_voxel)
    assert torch.equal(outs[0], outs[1])
    for b, plan in enumerate(plans):
        one = torch.full((T, 2, H, W), float("nan"), dtype=torch.float32, device=C.dev())
        ok(lib.ebos_iwe_voxel_owner_bwd_f32(P(plan.x), P(plan.y), P(plan.dt), None, P(plan.bins), P(plan.key_offsets), plan.n, P(voxels[b]), T,
                                            H, W, plan.tile[0], plan.tile[1], pad, pad, P(g_images[b]), P(affine[b]), g_lo, P(one), S()), lib)
        assert torch.equal(outs[0][b], one) and int(torch.count_nonzero(one)) > 0, b


@pytest.mark.parametrize("masked", [False, True])
def test_adjoint_adam_batch_is_the_single_call(lib, masked):
    gh, gw = C.O.patch_grid_shape((H, W), PATCH, PATCH)
    n_reg, cap, t = lib.ebos_flow_regularisers_partials(), 6, 3
    rs = np.random.RandomState(11)
    f32 = lambda a: G(a, torch.float32)  # noqa: E731
    d_dense = f32(rs.uniform(-1, 1, (B, 2, H, W)))
    theta0, m0, v0 = f32(rs.uniform(-2, 2, (B, 2, gh, gw))), f32(rs.uniform(-0.1, 0.1, (B, 2, gh, gw))), f32(rs.uniform(0, 0.01, (B, 2, gh, gw)))
    contrast, reg = f32(rs.uniform(1, 9, B)), G(rs.uniform(0, 1e-3, (B, n_reg)))
    mask = f32(rs.randint(0, 2, (B, gh, gw))) if masked else None
    scratch = torch.empty(B * (lib.ebos_upsample_bwd_scratch_bytes(gh, W) // 4), dtype=torch.float32, device=C.dev())
    geo = (gh, gw, *PATCH, *PATCH, H, W)
    adam = (0.05, 0.9, 0.999, 1e-8, t)
    outs = []
    for _ in range(2):
        bufs = [guarded((B, 2, gh, gw)) for _ in range(4)]
        (_, d_grid), (_, theta), (_, m), (_, v) = bufs
        theta.copy_(theta0), m.copy_(m0), v.copy_(v0)
        lbuf, losses = guarded((B, cap))
        step = torch.zeros(1, dtype=torch.int32, device=C.dev())
        ok(lib.ebos_upsample_patch_flow_bwd_adam_batch_f32(P(d_dense), B, *geo, P(scratch), P(d_grid), P(theta), P(m), P(v), *adam, P(step),
                                                           P(contrast), -1.5, P(reg), n_reg, P(losses), cap, P(mask), S()), lib)
        assert all(guards_untouched(b) for b, _ in bufs) and guards_untouched(lbuf) and int(step.item()) == t
        assert all(bool(torch.isfinite(x).all()) for x in (d_grid, theta, m, v)) and bool(torch.isfinite(losses[:, t - 1]).all())
        assert bool(torch.isnan(losses[:, :t - 1]).all()) and bool(torch.isnan(losses[:, t:]).all())    # one entry per window, no other
        outs.append((d_grid, theta, m, v, losses[:, t - 1].clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    for b in range(B):
        d1, th1, m1, v1 = torch.empty((2, gh, gw), dtype=torch.float32, device=C.dev()), theta0[b].clone(), m0[b].clone(), v0[b].clone()
        l1 = torch.full((cap,), float("nan"), dtype=torch.float32, device=C.dev())
        step = torch.zeros(1, dtype=torch.int32, device=C.dev())
        ok(lib.ebos_upsample_patch_flow_bwd_adam_f32(P(d_dense[b]), *geo, P(scratch), P(d1), P(th1), P(m1), P(v1), *adam, P(step),
                                                     P(contrast[b:]), -1.5, P(reg[b]), n_reg, P(l1), cap, P(None if mask is None else mask[b]),
                                                     S()), lib)
        got = [x[b] for x in outs[0][:4]]
        assert all(torch.equal(a, c) for a, c in zip(got, (d1, th1, m1, v1))), b
        assert torch.equal(outs[0][4][b], l1[t - 1]) and not torch.equal(th1, theta0[b]), b
        if masked:                                                # (a masked element's gradient is zero; its momentum still moves it)
            assert bool((d1[:, mask[b] == 0] == 0).all()) and bool((d1[:, mask[b] == 1] != 0).any())
    # the plain-gradient form: no step, nothing but d_grid written
    buf, d_grid = guarded((B, 2, gh, gw))
    ok(lib.ebos_upsample_patch_flow_bwd_batch_f32(P(d_dense), B, *geo, P(scratch), P(d_grid), S()), lib)
    assert guards_untouched(buf) and bool(torch.isfinite(d_grid).all())
    for b in range(B):
        d1 = torch.empty((2, gh, gw), dtype=torch.float32, device=C.dev())
        ok(lib.ebos_upsample_patch_flow_bwd_f32(P(d_dense[b]), *geo, P(scratch), P(d1), S()), lib)
        assert torch.equal(d_grid[b], d1), b


# ---------------------------------------------------------------------------------------------- 2. the tiled forward
def iwe_refs(windows, voxels):
    """float64 IWE of every window under its own voxel (cached by the caller's key)."""
    return [R.iwe_voxel(torch.from_numpy(ev), torch.from_numpy(np.ascontiguousarray(vx)), "first", True).numpy() for ev, vx in zip(windows, voxels)]


def stage_iwe_refs():
    return C.cached("batch_stage_iwe", lambda: iwe_refs(stage_windows(), stage_voxels()))


@pytest.mark.parametrize("halo,splits", [(HALO, 1), (HALO, 3), (8, 1), (24, 1)])     # (32, 32, 24) is no built configuration: the fall-back
def test_tiled_forward_batch_is_the_float64_iwe(ebos, lib, halo, splits):
    from event_based_bos_amd import _hip

    assert ((32, 32, halo) in set(_hip.tiled_configs())) == (halo != 24)
    _, stack = stack_of(ebos, stage_windows())
    voxels = G(np.stack(stage_voxels()), torch.float32).contiguous()
    buf, iwe = guarded((B, H, W), fill=float("nan"))
    iwe.zero_()                                                    # (the entry point accumulates)
    tiled_batch(lib, stack, voxels, halo, iwe, splits=splits)
    assert guards_untouched(buf)
    for b, want in enumerate(stage_iwe_refs()):
        print(f"halo {halo} splits {splits} window {b}: IWE relative L2 {rel(iwe[b], want):.3e}, mass {float(iwe[b].sum()):.1f}")
        assert rel(iwe[b], want) < 1e-4, b


def test_empty_window_in_the_batch(ebos, lib):
    """[w0, an empty window, w1]: row 1 of the offsets is constant (the window's base), ns[1] = 0.  Its image stays zero, every cell of
    its d_voxel is written with zero, and its neighbours get the bits of the batch without it."""
    windows = stage_windows()[:2]
    _, two = stack_of(ebos, windows)

    class WithEmpty(object):
        x, y, dt, bins, tile = two.x, two.y, two.dt, two.bins, two.tile
        ns = [two.ns[0], 0, two.ns[1]]
        key_offsets = torch.stack([two.key_offsets[0], torch.full_like(two.key_offsets[0], two.ns[0]), two.key_offsets[1]]).contiguous()

        def ns_array(self):
            return (ctypes.c_int64 * 3)(*self.ns)

        def __len__(self):
            return 3

    three = WithEmpty()
    voxels, g_images, affine = owner_inputs(T5, 0)
    iwe = torch.zeros((3, H, W), dtype=torch.float32, device=C.dev())
    tiled_batch(lib, three, voxels, HALO, iwe)
    refs = stage_iwe_refs()
    want = iwe_refs([windows[1]], [stage_voxels()[2]])[0]         # (w1 sits at index 2 here and reads voxel 2)
    assert int(torch.count_nonzero(iwe[1])) == 0 and rel(iwe[0], refs[0]) < 1e-4 and rel(iwe[2], want) < 1e-4
    buf, d3 = guarded((3, T5, 2, H, W))
    owner_batch(lib, three, voxels, g_images, affine, T5, 0, 0, d3)
    assert guards_untouched(buf) and bool(torch.isfinite(d3).all()) and int(torch.count_nonzero(d3[1])) == 0
    d2 = torch.empty((2, T5, 2, H, W), dtype=torch.float32, device=C.dev())
    owner_batch(lib, two, voxels[[0, 2]].contiguous(), g_images[[0, 2]].contiguous(), affine[[0, 2]].contiguous(), T5, 0, 0, d2)
    assert torch.equal(d3[0], d2[0]) and torch.equal(d3[2], d2[1])


# ---------------------------------------------------------------------------------------------- 3. window independence
def test_windows_are_independent_of_their_place_in_the_batch(ebos, lib):
    windows, refs = stage_windows(), stage_iwe_refs()
    voxels, g_images, affine = owner_inputs(T5, 0)
    # the plans are built once: the order of a pixel's events inside its run is a build's own (the counting sort ranks them with an
    # atomic counter), and the owner backward adds in that order
    plans = [C.plan_of(ebos, ev) for ev in windows]
    results = {}
    for order in ((0, 1, 2), (2, 0, 1)):
        idx = list(order)
        stack = ebos.EventPlan.stack_time_aware([plans[i] for i in idx])
        iwe = torch.zeros((B, H, W), dtype=torch.float32, device=C.dev())
        tiled_batch(lib, stack, voxels[idx].contiguous(), HALO, iwe)
        d_voxel = torch.full((B, T5, 2, H, W), float("nan"), dtype=torch.float32, device=C.dev())
        owner_batch(lib, stack, voxels[idx].contiguous(), g_images[idx].contiguous(), affine[idx].contiguous(), T5, 0, 0, d_voxel)
        for slot, i in enumerate(idx):
            results[(order, i)] = (iwe[slot], d_voxel[slot])
    for i in range(B):
        (iwe_a, dv_a), (iwe_b, dv_b) = results[((0, 1, 2), i)], results[((2, 0, 1), i)]
        assert torch.equal(dv_a, dv_b), i                           # the owner backward: the same bits wherever the window sits
        assert rel(iwe_a, refs[i]) < 1e-4 and rel(iwe_b, refs[i]) < 1e-4, i
    assert not torch.equal(results[((0, 1, 2), 0)][1], results[((0, 1, 2), 2)][1])


# ---------------------------------------------------------------------------------------------- 4. / 5. the loop
def thetas_start():
    """[B, 2, gh, gw]: a start grid per window (``C.theta_start`` with three seeds)."""
    return np.stack([C.theta_start(seed=81 + b) for b in range(B)])


def loop_windows(scheme, clamp=None):
    """[w0, w1, w2] kink-free under the float64 voxel of each window's own start grid."""
    def make():
        with torch.no_grad():
            voxels = [C.ref_voxel(torch.from_numpy(th).double(), scheme, clamp)[1].numpy() for th in thetas_start()]
        return three_windows(voxels, seed=53)
    return C.cached(("batch_loop_windows", scheme, clamp), make)


def ref_value_and_grad(b, scheme, clamp, w_norm, w_tv):
    """(loss, d loss / d theta) of window b at its start grid: the float64 objective through autograd (``C.ref_loss``)."""
    def make():
        th = torch.from_numpy(thetas_start()[b]).double().requires_grad_(True)
        loss = C.ref_loss(th, loop_windows(scheme, clamp)[b], scheme, clamp, w_norm, w_tv)
        loss.backward()
        return loss.item(), th.grad.numpy()
    return C.cached(("batch_loop_grad", b, scheme, clamp, w_norm, w_tv), make)


def ref_adam_losses(b, scheme, n_iter, lr=0.05):
    """``n_iter`` iterations of torch.optim.Adam on window b's float64 objective from its start grid: the losses before each update."""
    def make():
        th = torch.from_numpy(thetas_start()[b]).double().requires_grad_(True)
        opt = torch.optim.Adam([th], lr=lr)
        out = []
        for _ in range(n_iter):
            opt.zero_grad(set_to_none=True)
            loss = C.ref_loss(th, loop_windows(scheme)[b], scheme)
            loss.backward()
            opt.step()
            out.append(loss.item())
        return out
    return C.cached(("batch_loop_adam", b, scheme, n_iter, lr), make)


def time_aware(scheme, clamp=None):
    return {"time_bin": T5, "scheme": scheme, "t0_location": "middle", "clamp": clamp, "native": True}


def make_batch_loop(ebos, windows, scheme, clamp=None, w_norm=0.0, w_tv=0.0, capacity=8, **kw):
    from event_based_bos_amd.solver.time_aware_loop import TimeAwarePatchLoopBatch

    plans = [C.plan_of(ebos, ev) for ev in windows]
    return TimeAwarePatchLoopBatch(plans, PATCH, PATCH, G(thetas_start()), time_aware(scheme, clamp), 1.0, w_norm, w_tv, lr=0.05,
                                   capacity=capacity, **kw)


# one combination per axis: both schemes, with and without the two regularisers, clamp None and 2.0, both backwards
@pytest.mark.parametrize("scheme,reg,clamp,owner", [("upwind", 0.0, None, 1), ("burgers", 0.1, None, 0), ("upwind", 0.1, 2.0, 0),
                                                    ("burgers", 0.0, 2.0, 1)])
def test_batch_loop_first_iteration_is_float64_autograd(ebos, scheme, reg, clamp, owner):
    windows = loop_windows(scheme, clamp)
    loop = make_batch_loop(ebos, windows, scheme, clamp, reg, reg, owner_bwd=bool(owner))
    start = loop.theta.clone()
    losses = loop.run(1)
    assert loop.last_run_mode == "native-batch" and loop.t == 1 and int(loop.step.item()) == 1 and losses.shape == (B, 1)
    assert loop.theta.shape == start.shape and loop.d_theta.shape == start.shape and loop.losses.shape == (B, 8)
    value, grad = None, None
    for b in range(B):
        loss_ref, grad_ref = ref_value_and_grad(b, scheme, clamp, reg, reg)
        print(f"{scheme} reg={reg} clamp={clamp} owner_bwd={owner} window {b}: loss rel {abs(losses[b, 0].item() - loss_ref) / abs(loss_ref):.3e}, "
              f"d_theta rel L2 {rel(loop.d_theta[b], grad_ref):.3e}")
        assert abs(losses[b, 0].item() - loss_ref) < 1e-5 * abs(loss_ref) and rel(loop.d_theta[b], grad_ref) < 1e-3, b
        assert not torch.equal(loop.theta[b], start[b])                              # Adam moved every window's grid
    # value_and_grad: the same kernels without the step, at the start
    value, grad = loop.value_and_grad(start)
    assert value.shape == (B,) and grad.shape == start.shape and torch.equal(loop.theta, start)
    for b in range(B):
        loss_ref, grad_ref = ref_value_and_grad(b, scheme, clamp, reg, reg)
        assert abs(value[b].item() - loss_ref) < 1e-5 * abs(loss_ref) and rel(grad[b], grad_ref) < 1e-3, b


def test_owner_backward_default_and_refusals(ebos):
    from event_based_bos_amd.solver.time_aware_loop import TimeAwarePatchLoopBatch, default_owner_bwd

    windows = loop_windows("upwind")
    loop = make_batch_loop(ebos, windows, "upwind")
    assert loop.owner_bwd == default_owner_bwd(T5, max(len(w) for w in windows)) and loop.B == B
    with pytest.raises(ValueError, match="capacity"):
        loop.run(9)
    plans = [C.plan_of(ebos, ev) for ev in windows]
    with pytest.raises(ValueError, match="theta0"):
        TimeAwarePatchLoopBatch(plans, PATCH, PATCH, G(thetas_start()[:2]), time_aware("upwind"))
    with pytest.raises(ValueError, match="time_bin"):
        TimeAwarePatchLoopBatch(plans, PATCH, PATCH, G(thetas_start()), dict(time_aware("upwind"), time_bin=15))
    with pytest.raises(ValueError, match="tile"):
        ebos.EventPlan.stack_time_aware([plans[0], C.plan_of(ebos, windows[1], tile=(64, 64))])


def test_five_iterations_follow_the_float64_adam_loop(ebos):
    from event_based_bos_amd.solver.time_aware_loop import TimeAwarePatchLoop

    windows = loop_windows("upwind")
    want = np.array([ref_adam_losses(b, "upwind", 5) for b in range(B)])
    # for the record, the single-window loop on each window (what SINGLE_LOOP_DEVIATION was measured with)
    for b, ev in enumerate(windows):
        one = TimeAwarePatchLoop(C.plan_of(ebos, ev), PATCH, PATCH, G(thetas_start()[b]), time_aware("upwind"), 1.0, lr=0.05, capacity=8,
                                 owner_bwd=True)
        got = one.run(5).cpu().numpy().astype(np.float64)
        print(f"single loop, window w{b}, deviation per iteration:", (np.abs(got - want[b]) / np.abs(want[b])).tolist())
    loop = make_batch_loop(ebos, windows, "upwind", owner_bwd=True)
    got = loop.run(5).cpu().numpy().astype(np.float64)
    assert got.shape == (B, 5)
    dev = np.abs(got - want) / np.abs(want)
    for b in range(B):
        print(f"batch loop, window w{b}, deviation per iteration:", dev[b].tolist())
    for b in range(B):
        bound = BATCH_LOOP_FACTOR * max(SINGLE_LOOP_DEVIATION[f"w{b}"])
        assert want[b, -1] < want[b, 0] and got[b, -1] < got[b, 0], b                # the loss falls
        assert (dev[b] <= bound).all(), (b, dev[b], bound)


# ---------------------------------------------------------------------------------------------- 6. the solver
def solver_windows(seed=61):
    def make():
        w0 = C.O.synth_events(N, H, W, seed=seed, tmin=0.0, tmax=1.0)
        w0[0, 2], w0[-1, 2] = 0.0, 1.0
        w1 = np.concatenate([w0[:1], w0[1:-1][::3], w0[-1:]])
        return [w0, w1, C.with_hot_pixel(w0, np.zeros((T5, 2, H, W)))]
    return C.cached(("batch_solver_windows", seed), make)


def tolerance(b):
    return BATCH_LOOP_FACTOR * max(SINGLE_LOOP_DEVIATION[f"w{b}"])


@pytest.mark.parametrize("pyramid", [False, True])
def test_solver_estimate_batch(ebos, pyramid):
    windows = solver_windows()
    cfg = C.solver_config(True, n_iter=5)
    if pyramid:                                                   # two scales, and patches with too few events are not estimated
        cfg["patch"] = {"pyramid": {"coarsest": 16, "finest": 8}, "do_event_thresholding": True, "event_thres": 120}
    make = ebos.solver.collections["contrast_maximization"]
    singles = []
    for ev in windows:
        slv = make((H, W), (H, W), solver_config=cfg)
        if not pyramid:
            slv.previous_best = C.theta_start() * 0.2             # the warm start is every window's start
        singles.append((slv.estimate(ev), list(slv.history), slv.patch_flow.clone()))
        assert slv.loop_mode == "native"
    results = {}
    for max_batch in (8, 2):
        slv = make((H, W), (H, W), solver_config=cfg)
        if not pyramid:
            slv.previous_best = C.theta_start() * 0.2
        flows = slv.estimate_batch(windows, max_batch=max_batch)
        n_scales = len(slv.pyramid_scales())
        assert flows.shape == (B, 2, H, W) and flows.dtype == np.float64 and np.isfinite(flows).all()
        assert slv.loop_modes == ["native-batch"] * n_scales and n_scales == (2 if pyramid else 1) and slv.loop_mode == "native-batch"
        assert len(slv.histories) == B and len(slv.patch_flows) == B and slv.history == slv.histories[-1]
        assert torch.equal(slv.patch_flow, slv.patch_flows[-1])
        for b in range(B):
            flow1, hist1, theta1 = singles[b]
            assert len(slv.histories[b]) == sum(n for _, _, n in slv.pyramid_scales()) == len(hist1)
            dev = np.abs(np.array(slv.histories[b]) - np.array(hist1)) / np.abs(np.array(hist1))
            print(f"pyramid={pyramid} max_batch={max_batch} window {b}: history deviation {dev.tolist()}, flow rel L2 {rel(flows[b], flow1):.3e}")
            assert (dev <= tolerance(b)).all(), (b, dev, tolerance(b))
            assert rel(flows[b], flow1) < 1e-3 and rel(slv.patch_flows[b], theta1) < 1e-3, b
        results[max_batch] = (flows, [list(h) for h in slv.histories])
        if pyramid:                                               # the masks are each window's own
            plan = ebos.EventPlan.build(G(windows[1]), (H, W), "first", True, tile=C.TILE, emit="full", time_bin=T5)
            mask = slv.patch_mask(plan, (8, 8), (8, 8)).cpu().numpy()
            theta = slv.patch_flows[1].cpu().numpy()
            assert (mask == 0).any() and (mask == 1).any() and (theta[:, mask == 0] == 0).all() and (theta[:, mask == 1] != 0).any()
    for b in range(B):                                            # chunks of two give what one chunk of three gives
        dev = np.abs(np.array(results[2][1][b]) - np.array(results[8][1][b])) / np.abs(np.array(results[8][1][b]))
        assert (dev <= tolerance(b)).all() and rel(results[2][0][b], results[8][0][b]) < 1e-3, (b, dev)
