"""GPU tests of the native time-aware loop: the pixel-owner backward into the flow voxel (``ebos_iwe_voxel_owner_bwd_f32`` through
``EventPlan.variance_voxel_value_and_grad``), the loop of one C call (``TimeAwarePatchLoop``: the batch loop with one window; the C
entry points of one window, ``ebos_cmax_voxel_solve_f32`` / ``_gradient_f32``, by hand) and the solver's ``time_aware.native`` switch.  Yardsticks and windows: tests/_voxel_loop_cases.py (CPU, float64, torch autograd).  Bars are the
project's: values relative < 1e-5, gradients relative L2 < 1e-3."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxel_loop_cases as C  # noqa: E402
from _voxel_loop_cases import G, H, N, PATCH, R, T5, W, rel  # noqa: E402

pytestmark = pytest.mark.gpu

# Test 7's tolerance.  How far the autograd loop of the solver (``time_aware`` without ``native``: the loop this one replaces) lies from
# the float64 CPU loop on the same window from the same start, |loss - loss64| / |loss64| per iteration, measured on an MI355X (the test
# prints them again on every run); in that run the native loop's five losses were the autograd loop's bit for bit, with either backward:
AUTOGRAD_LOOP_DEVIATION = (6.91e-08, 1.13e-08, 2.47e-08, 3.69e-08, 4.56e-08)
# The native loop runs the same float32 kernels in another summation order, and the few events that cross a kink of the vote between
# two iterations break their ties alike in both: it is allowed twice that.  "That" is the largest of the five: each of them is the
# rounding of one float32 loss near -7 (half a unit in the last place is 3.4e-8 there), so twice the smaller ones would ask a float32
# number to lie closer to the float64 one than the format's own step, which the forward kernel's float atomics do not promise.
NATIVE_LOOP_FACTOR = 2.0


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


# ---------------------------------------------------------------------------------------------- the owner backward
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("omit", [False, True])
def test_owner_backward_is_float64_autograd(ebos, omit, pad, T):
    vx, ev = C.voxel_u(6.0, T), C.kink_free(T)
    var_ref, dv_ref = C.ref_variance_grad(("kf", T), ev, vx, omit, pad)
    plan = C.plan_of(ebos, ev, T=T)
    value, d_voxel = plan.variance_voxel_value_and_grad(G(vx, torch.float32), omit, pad=(pad, pad))
    print(f"omit={omit} pad={pad} T={T}: value rel {abs(value.item() - var_ref) / var_ref:.3e}, d_voxel rel L2 {rel(d_voxel, dv_ref):.3e}")
    assert value.shape == (1,) and d_voxel.shape == (T, 2, H, W) and d_voxel.dtype == torch.float32
    assert abs(value.item() - var_ref) < 1e-5 * var_ref and rel(d_voxel, dv_ref) < 1e-3
    # upstream scales the gradient, not the value; the autograd route gives the same gradient
    v2, d2 = plan.variance_voxel_value_and_grad(G(vx, torch.float32), omit, pad=(pad, pad), upstream=-0.5)
    assert torch.equal(v2, value) and rel(d2, -0.5 * dv_ref) < 1e-3
    v = G(vx, torch.float32).requires_grad_(True)
    plan.contrast_voxel(v, "image_variance", omit, pad=(pad, pad)).backward()
    assert rel(d_voxel, v.grad) < 1e-4


def test_owner_backward_writes_every_cell(ebos):
    vx, ev = C.voxel_u(6.0), C.kink_free(empty_bin=3)
    assert not (R.time_bins(ev[:, 2], T5) == 3).any()
    _, dv_ref = C.ref_variance_grad("e3", ev, vx, False, 0)
    plan = C.plan_of(ebos, ev)
    out = torch.full((T5, 2, H, W), float("nan"), dtype=torch.float32, device=C.dev())
    _, d_voxel = plan.variance_voxel_value_and_grad(G(vx, torch.float32), out=out)
    assert d_voxel is out and bool(torch.isfinite(out).all())                        # nothing of the NaN fill is left
    assert int(torch.count_nonzero(out[3])) == 0                                     # a bin without events: exactly zero
    assert rel(out, dv_ref) < 1e-3
    # the rows and columns of the tiles that overhang the 37 x 70 image (tile 32 x 32: rows 32.., columns 64..)
    got = out.cpu().numpy()
    assert np.abs(dv_ref[:, :, 32:, :]).max() > 0 and np.abs(dv_ref[:, :, :, 64:]).max() > 0
    assert rel(got[:, :, 32:, :], dv_ref[:, :, 32:, :]) < 1e-3 and rel(got[:, :, :, 64:], dv_ref[:, :, :, 64:]) < 1e-3
    # a window that leaves whole tiles empty: their pixels are written too
    left = ev[ev[:, 1] < 30].copy()
    left[0, 2], left[-1, 2] = 0.0, 1.0
    _, dl_ref = C.ref_variance_grad("e3-left", left, vx, False, 0)
    out.fill_(float("nan"))
    C.plan_of(ebos, left).variance_voxel_value_and_grad(G(vx, torch.float32), out=out)
    assert bool(torch.isfinite(out).all()) and int(torch.count_nonzero(out[:, :, :, 32:])) == 0 and rel(out, dl_ref) < 1e-3
    # out has to be what the kernel can fill, and the plan a binned time-aware one
    with pytest.raises(ValueError):
        plan.variance_voxel_value_and_grad(G(vx, torch.float32), out=torch.empty((T5, 2, H, W), dtype=torch.float64, device=C.dev()))
    with pytest.raises(ValueError):
        plan.variance_voxel_value_and_grad(G(C.voxel_u(6.0, 1), torch.float32))       # a voxel of 1 bin on a plan of 5
    with pytest.raises(ValueError):
        ebos.EventPlan.build(G(ev), (H, W), tile=C.TILE).variance_voxel_value_and_grad(G(vx, torch.float32))   # a plan without bins
    with pytest.raises(NotImplementedError):
        C.plan_of(ebos, ev, tile=None).variance_voxel_value_and_grad(G(vx, torch.float32))                      # un-binned


def hot_window():
    vx = C.voxel_u(6.0)
    return vx, C.cached("hot", lambda: C.with_hot_pixel(C.kink_free(), vx))


def test_owner_backward_is_reproducible(ebos):
    """Two calls of the kernel on one plan with the same inputs: the same bits.  The upstream image is made once: the forward kernel
    sums the tiles' windows into the IWE with float atomics, so two IWEs of one voxel may differ in their last bits, and a gradient
    cannot repeat more exactly than what it is given (``variance_voxel_value_and_grad`` twice: printed, not judged)."""
    from event_based_bos_amd import _hip
    from event_based_bos_amd._hip import ptr, stream_ptr

    vx, ev = hot_window()                                                            # short runs and the wave's path
    plan = C.plan_of(ebos, ev)
    v = G(vx, torch.float32)
    iwe = plan.iwe_voxel(v).contiguous()
    affine = torch.tensor([0.37, -0.11], dtype=torch.float32, device=C.dev())
    outs = [torch.full((T5, 2, H, W), fill, dtype=torch.float32, device=C.dev()) for fill in (float("nan"), 7.0)]
    for out in outs:
        _hip.check(_hip.require_gpu().ebos_iwe_voxel_owner_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), None, ptr(plan.bins),
                                                                   ptr(plan.key_offsets), plan.n, ptr(v), T5, H, W, plan.tile[0], plan.tile[1],
                                                                   0, 0, ptr(iwe), ptr(affine), 0, ptr(out), stream_ptr()),
                   "ebos_iwe_voxel_owner_bwd")
    assert torch.equal(outs[0], outs[1]) and int(torch.count_nonzero(outs[0])) > 0
    a, b = plan.variance_voxel_value_and_grad(v)[1], plan.variance_voxel_value_and_grad(v)[1]
    print("through two forward passes: bit-identical" if torch.equal(a, b) else f"through two forward passes: relative L2 {rel(a, b):.3e}")


def test_hot_pixel_with_bins_out_of_order(ebos):
    vx, ev = hot_window()
    assert len(ev) == N + C.HOT_EXTRA
    var_ref, dv_ref = C.ref_variance_grad("hot", ev, vx, False, 0)
    plan = C.plan_of(ebos, ev)
    r, c = C.HOT_PIXEL
    key = ((r // 32) * 3 + c // 32) * 1024 + (r % 32) * 32 + c % 32                   # 2 x 3 tiles of 32 x 32
    ko = plan.key_offsets.cpu().numpy()
    run = plan.bins.cpu().numpy()[ko[key]:ko[key + 1]].astype(np.int64)
    assert len(run) >= C.HOT_EXTRA and (np.diff(run) < 0).any() and set(run) == set(range(T5))   # one long run, its bins unsorted
    value, d_voxel = plan.variance_voxel_value_and_grad(G(vx, torch.float32))
    print(f"hot pixel: value rel {abs(value.item() - var_ref) / var_ref:.3e}, d_voxel rel L2 {rel(d_voxel, dv_ref):.3e}")
    assert abs(value.item() - var_ref) < 1e-5 * var_ref and rel(d_voxel, dv_ref) < 1e-3
    got, want = d_voxel[:, :, r, c].cpu().numpy().astype(np.float64), dv_ref[:, :, r, c]
    print("the pixel's ten cells, relative:", np.abs(got - want) / np.abs(want))
    assert (np.abs(got - want) < 1e-3 * np.abs(want)).all()


def test_255_bins_and_a_bins_array_made_for_more_bins(ebos):
    """8 x 9 image, 300 events, T = 255: a single tile that overhangs the image on both sides, most bins empty or holding one
    event.  Then the C entry with T = 100 on the plan's bins, which were made for 255: the kernel reads min(bin, T - 1)."""
    h, w, n, T = 8, 9, 300, 255
    vx = C.voxel_u(2.0, T, seed=23, shape=(h, w))
    rs = np.random.RandomState(91)
    pool = np.stack([rs.uniform(0, h, 2 * n), rs.uniform(0, w, 2 * n), np.sort(rs.uniform(0, 1, 2 * n)), rs.randint(0, 2, 2 * n)], axis=1)
    pool[0, 2], pool[-1, 2] = 0.0, 1.0
    g_np = rs.uniform(-1, 1, (h, w))

    def off_kinks(vox, bins=None):
        warped = R.warp_voxel(torch.from_numpy(pool), torch.from_numpy(vox), "first", True, bins=bins)[0].numpy()
        return ~(np.abs(warped[:, :2] - np.rint(warped[:, :2])) < 5e-4).any(1)

    bins100 = torch.from_numpy(np.minimum(R.time_bins(pool[:, 2], T), 99))[None]
    ok = off_kinks(vx) & off_kinks(vx[:100], bins100)
    ok[0] = ok[-1] = True
    ev = np.concatenate([pool[:-1][ok[:-1]][:n - 1], pool[-1:]])
    assert len(ev) == n
    plan = C.plan_of(ebos, ev, T=T, shape=(h, w))
    assert plan.n == n and int(plan.bins.max()) == T - 1
    v64 = torch.from_numpy(vx).clone().requires_grad_(True)
    var = R.image_variance(R.iwe_voxel(torch.from_numpy(ev), v64, "first", True))
    var.backward()
    value, d_voxel = plan.variance_voxel_value_and_grad(G(vx, torch.float32))
    print(f"T = 255: value rel {abs(value.item() - var.item()) / var.item():.3e}, d_voxel rel L2 {rel(d_voxel, v64.grad):.3e}")
    assert abs(value.item() - var.item()) < 1e-5 * var.item() and rel(d_voxel, v64.grad) < 1e-3
    # T = 100 on bins made for 255, an explicit upstream image, and guard cells around d_voxel that must stay as they are
    from event_based_bos_amd import _hip
    from event_based_bos_amd._hip import ptr, stream_ptr
    Tc, cells, guard = 100, 100 * 2 * h * w, 4096
    buf = torch.full((guard + cells + guard,), float("nan"), dtype=torch.float32, device=C.dev())
    v32, g32 = G(vx[:Tc], torch.float32).contiguous(), G(g_np, torch.float32)
    out = buf[guard:guard + cells]
    _hip.check(_hip.require_gpu().ebos_iwe_voxel_owner_bwd_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), None, ptr(plan.bins), ptr(plan.key_offsets),
                                                               plan.n, ptr(v32), Tc, h, w, plan.tile[0], plan.tile[1], 0, 0, ptr(g32), None, 0,
                                                               out.data_ptr(), stream_ptr()), "ebos_iwe_voxel_owner_bwd")
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + cells:]).all()) and bool(torch.isfinite(out).all())
    v64 = torch.from_numpy(vx[:Tc]).clone().requires_grad_(True)
    clamped = torch.from_numpy(np.minimum(R.time_bins(ev[:, 2], T), Tc - 1))[None]
    (R.iwe_voxel(torch.from_numpy(ev), v64, "first", True, bins=clamped) * torch.from_numpy(g_np)).sum().backward()
    print(f"T = 100 on bins for 255: d_voxel rel L2 {rel(out.reshape(Tc, 2, h, w), v64.grad):.3e}")
    assert rel(out.reshape(Tc, 2, h, w), v64.grad) < 1e-3


# ---------------------------------------------------------------------------------------------- the loop
def make_loop(ebos, ev, scheme, clamp=None, w_norm=0.0, w_tv=0.0, capacity=8, **kw):
    from event_based_bos_amd.solver.time_aware_loop import TimeAwarePatchLoop

    ta = {"time_bin": T5, "scheme": scheme, "t0_location": "middle", "clamp": clamp, "native": True}
    return TimeAwarePatchLoop(C.plan_of(ebos, ev), PATCH, PATCH, G(C.theta_start()), ta, 1.0, w_norm, w_tv, lr=0.05, capacity=capacity, **kw)


@pytest.mark.parametrize("clamp", [None, 2.0])
@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("scheme", ["upwind", "burgers"])
def test_loop_first_iteration_is_float64_autograd(ebos, scheme, reg, clamp):
    ev = C.loop_events(scheme, clamp)
    loss_ref, grad_ref = C.ref_value_and_grad(ev, scheme, clamp, reg, reg)
    for owner in (1, 0):
        loop = make_loop(ebos, ev, scheme, clamp, reg, reg, owner_bwd=bool(owner))
        start = loop.theta.clone()
        losses = loop.run(1)
        assert loop.last_run_mode == "native" and loop.t == 1 and int(loop.step.item()) == 1 and losses.shape == (1,)
        print(f"{scheme} reg={reg} clamp={clamp} owner_bwd={owner}: loss rel {abs(losses[0].item() - loss_ref) / abs(loss_ref):.3e}, "
              f"d_theta rel L2 {rel(loop.d_theta, grad_ref):.3e}")
        assert abs(losses[0].item() - loss_ref) < 1e-5 * abs(loss_ref) and rel(loop.d_theta, grad_ref) < 1e-3
        assert not torch.equal(loop.theta, start)                                    # Adam moved the grid
        # value_and_grad: the same kernels without the step, at the start
        value, grad = loop.value_and_grad(start)
        assert abs(value.item() - loss_ref) < 1e-5 * abs(loss_ref) and rel(grad, grad_ref) < 1e-3 and torch.equal(loop.theta, start)


def test_loop_five_iterations_follow_the_float64_adam_loop(ebos):
    ev = C.loop_events("upwind")
    want = np.array(C.ref_adam_losses(ev, "upwind", 5))
    # the loop this one replaces, for the record: the solver without ``native``, the same window, the same start
    slv = ebos.solver.collections["contrast_maximization"]((H, W), (H, W), solver_config=C.solver_config(None))
    slv.previous_best = C.theta_start()
    slv.estimate(ev)
    assert slv.loop_mode == "autograd"
    print("autograd loop, deviation per iteration:", (np.abs(np.array(slv.history) - want) / np.abs(want)).tolist())
    for owner in (1, 0):
        loop = make_loop(ebos, ev, "upwind", owner_bwd=bool(owner))
        got = loop.run(5).cpu().numpy().astype(np.float64)
        dev = np.abs(got - want) / np.abs(want)
        print(f"native loop (owner_bwd={owner}), deviation per iteration:", dev.tolist())
        assert want[-1] < want[0] and got[-1] < got[0]                               # the loss falls
        assert (dev <= NATIVE_LOOP_FACTOR * max(AUTOGRAD_LOOP_DEVIATION)).all(), (dev, AUTOGRAD_LOOP_DEVIATION)


def single_problem(loop, **over):
    """``ebos_cmax_voxel_problem`` of a one-window loop's buffers: the batch problem's fields copied by name, ``n`` from ``n[0]``."""
    from event_based_bos_amd import _hip

    batch, q = loop.problem(), _hip.CmaxVoxelProblem()
    assert batch.B == 1
    for name, _ in q._fields_:
        setattr(q, name, batch.n[0] if name == "n" else getattr(batch, name))
    for name, value in over.items():
        setattr(q, name, value)
    return q


# both regularisers and a clamp with the owner backward; neither with the atomic backward; halo 24, which is no built configuration:
# the tiled batch entry point finds no kernel for it and runs the general forward kernel
@pytest.mark.parametrize("reg,clamp,owner,halo", [(0.1, 2.0, 1, None), (0.0, None, 0, None), (0.0, None, 1, 24)])
def test_single_c_entry_points_are_float64_autograd(ebos, reg, clamp, owner, halo):
    """``ebos_cmax_voxel_gradient_f32`` and one iteration of ``ebos_cmax_voxel_solve_f32``, which Python no longer calls."""
    import ctypes

    from event_based_bos_amd import _hip

    lib = _hip.require_gpu()
    if halo is not None:
        assert (C.TILE[0], C.TILE[1], halo) not in set(_hip.tiled_configs())
    ev = C.loop_events("upwind", clamp)
    loss_ref, grad_ref = C.ref_value_and_grad(ev, "upwind", clamp, reg, reg)
    loop = make_loop(ebos, ev, "upwind", clamp, reg, reg, owner_bwd=bool(owner))
    start = loop.theta.clone()
    q = single_problem(loop, **({} if halo is None else {"halo": halo}))
    assert q.n == len(ev) and q.owner_bwd == owner and q.has_clamp == int(clamp is not None)
    loop.d_theta.fill_(float("nan"))
    _hip.check(lib.ebos_cmax_voxel_gradient_f32(ctypes.byref(q), _hip.stream_ptr()), "ebos_cmax_voxel_gradient")
    value = -loop.variance[0].item() + (loop.reg_partials.sum().item() if reg else 0.0)
    print(f"gradient entry, reg={reg} clamp={clamp} owner_bwd={owner} halo={halo}: loss rel {abs(value - loss_ref) / abs(loss_ref):.3e}, "
          f"d_theta rel L2 {rel(loop.d_theta, grad_ref):.3e}")
    assert abs(value - loss_ref) < 1e-5 * abs(loss_ref) and rel(loop.d_theta, grad_ref) < 1e-3
    assert torch.equal(loop.theta, start) and int(loop.step.item()) == 0               # no step
    loop.d_theta.fill_(float("nan"))
    _hip.check(lib.ebos_cmax_voxel_solve_f32(ctypes.byref(q), 1, _hip.stream_ptr()), "ebos_cmax_voxel_solve")
    loss = loop.losses[0].item()
    print(f"solve entry, reg={reg} clamp={clamp} owner_bwd={owner} halo={halo}: loss rel {abs(loss - loss_ref) / abs(loss_ref):.3e}, "
          f"d_theta rel L2 {rel(loop.d_theta, grad_ref):.3e}")
    assert abs(loss - loss_ref) < 1e-5 * abs(loss_ref) and rel(loop.d_theta, grad_ref) < 1e-3
    assert int(loop.step.item()) == 1 and not torch.equal(loop.theta, start)          # Adam moved the grid


def test_one_window_face_of_the_batch_loop(ebos):
    """``TimeAwarePatchLoop`` is a batch loop of one window without the window dimension; its state tensors are views of the buffers
    the kernels read, so the reset of tools/bench_voxel_loop.py starts the same solve again."""
    ev = C.loop_events("upwind")
    want = np.array(C.ref_adam_losses(ev, "upwind", 5))[:3]
    bound = NATIVE_LOOP_FACTOR * max(AUTOGRAD_LOOP_DEVIATION)
    loop = make_loop(ebos, ev, "upwind", owner_bwd=True)
    gh, gw = C.theta_start().shape[1:]
    assert loop.theta.shape == loop.d_theta.shape == loop.exp_avg.shape == loop.exp_avg_sq.shape == (2, gh, gw)
    assert loop.losses.shape == (8,) and loop.batch.B == 1 and loop.theta.data_ptr() == loop.batch.theta.data_ptr()
    assert loop.last_run_mode == "native" and loop.graphed is False and loop.owner_bwd is True and loop.t == 0
    start = loop.theta.clone()
    first = loop.run(3).clone()
    assert first.shape == (3,) and loop.t == 3 and int(loop.step.item()) == 3 and not torch.equal(loop.theta, start)
    loop.theta.copy_(start)
    loop.exp_avg.zero_()
    loop.exp_avg_sq.zero_()
    loop.t = 0
    second = loop.run(3)
    assert second.shape == (3,) and loop.t == 3 and loop.batch.t == 3
    print("two runs of three iterations from one start:", "bit-identical" if torch.equal(first, second) else
          f"relative difference {((first - second).abs() / second.abs()).tolist()}")
    for name, got in (("first", first), ("second", second)):
        dev = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.abs(want)
        print(f"{name} run, deviation per iteration:", dev.tolist())
        assert (dev <= bound).all(), (name, dev, bound)


# ---------------------------------------------------------------------------------------------- the solver
def events_int(seed=61):
    return C.cached(("ev_int", seed), lambda: C.O.synth_events(N, H, W, seed=seed, tmin=0.0, tmax=1.0))


def test_solver_native_switch(ebos):
    from event_based_bos_amd.solver.contrast_maximization import patch_grid_shape
    from event_based_bos_amd.solver.time_aware_loop import TimeAwarePatchLoop

    ev = events_int()
    make = ebos.solver.collections["contrast_maximization"]
    slv = make((H, W), (H, W), solver_config=C.solver_config(True, tile=None))
    assert slv.plan_tile() == (64, 64)
    flow = slv.estimate(ev)
    assert flow.shape == (2, H, W) and np.isfinite(flow).all() and np.isfinite(slv.history).all()
    assert slv.loop_mode == "native" and slv.loop_modes == ["native"] and slv.fused and not slv.graphed and len(slv.history) == 5
    # the same loop driven by hand on the same plan
    plan = ebos.EventPlan.build(G(ev), (H, W), "first", True, tile=slv.plan_tile(), emit="full", time_bin=T5)
    gh, gw = patch_grid_shape((H, W), PATCH, PATCH)
    loop = TimeAwarePatchLoop(plan, PATCH, PATCH, torch.zeros((2, gh, gw), device=C.dev()), slv.time_aware, 1.0, lr=0.05, capacity=5)
    history = loop.run(5).cpu().tolist()
    print("solver", slv.history, "by hand", history)
    assert np.allclose(slv.history, history, rtol=1e-5, atol=0.0)
    # ... and the autograd loop of the same configuration computes the same objective
    off = make((H, W), (H, W), solver_config=C.solver_config(False, tile=None))
    off.estimate(ev)
    assert off.loop_mode == "autograd" and not off.fused and len(off.history) == 5
    assert abs(off.history[0] - slv.history[0]) < 1e-5 * abs(off.history[0])
    # a pyramid: every scale runs the native loop
    pyr = C.solver_config(True, n_iter=6)
    pyr["patch"] = {"pyramid": {"coarsest": 16, "finest": 8}}
    slv = make((H, W), (H, W), solver_config=pyr)
    slv.estimate(ev)
    assert slv.loop_modes == ["native", "native"] and slv.loop_mode == "native" and slv.fused
    assert len(slv.history) == sum(n for _, _, n in slv.pyramid_scales()) and np.isfinite(slv.history).all()


def test_solver_native_event_threshold_and_scipy(ebos):
    make = ebos.solver.collections["contrast_maximization"]
    ev = events_int()
    # event_thres: the patches of the emptied columns are not estimated and stay exactly at zero
    part = ev[ev[:, 1] < 50].copy()
    part[0, 2], part[-1, 2] = 0.0, 1.0
    cfg = C.solver_config(True)
    cfg["patch"].update({"do_event_thresholding": True, "event_thres": 100})
    slv = make((H, W), (H, W), solver_config=cfg)
    slv.estimate(part)
    plan = ebos.EventPlan.build(G(part), (H, W), "first", True, tile=C.TILE, emit="full", time_bin=T5)
    mask = slv.patch_mask(plan, PATCH, PATCH).cpu().numpy()
    theta = slv.patch_flow.cpu().numpy()
    assert slv.loop_mode == "native" and (mask == 0).any() and (mask == 1).any()
    assert (theta[:, mask == 0] == 0).all() and (theta[:, mask == 1] != 0).any()
    # L-BFGS-B from a warm start, through value_and_grad
    cfg = C.solver_config(True)
    cfg["optimizer"] = {"method": "L-BFGS-B", "n_iter": 5}
    slv = make((H, W), (H, W), solver_config=cfg)
    slv.previous_best = C.theta_start() * 0.2
    slv.estimate(ev)
    print("L-BFGS-B", slv.history[0], "->", float(slv.scipy_result.fun), f"in {len(slv.history)} evaluations")
    assert slv.loop_mode == "native" and slv.fused and len(slv.history) >= 2 and float(slv.scipy_result.fun) < slv.history[0]
