"""GPU tests of the multi-reference contrast: the fused IWEs at several reference times (``ebos_iwe_dense_multiref_tiled_f32``), their
owner backward (``ebos_iwe_dense_multiref_owner_bwd_f32``), the loop route, ``EventPlan.iwe_dense_multi`` / ``contrast_dense_multi`` and
the solver's ``multi_reference`` block.  Yardsticks and windows: tests/_multiref_cases.py (CPU, float64, torch autograd).  Bars are the
project's: IWE relative L2 < 1e-4, values relative < 1e-5, gradients relative L2 < 1e-3."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multiref_cases as C  # noqa: E402
from _multiref_cases import BMA, FML, FQML, G, H, N, PATCH, W, rel  # noqa: E402

pytestmark = pytest.mark.gpu

# The tolerance of test_solver_adam_loop_follows_the_float64_loop.  How far the EXISTING single-reference autograd loop of the solver
# (no ``multi_reference`` block, ``optimizer.fused`` and ``optimizer.graph`` off: the code path of the parent commit) lies from its own
# float64 CPU loop on this window from the same start, |loss - loss64| / |loss64| per iteration, measured on an MI355X (the test
# prints them again on every run):
SINGLE_REFERENCE_LOOP_DEVIATION = (8.35e-08, 9.71e-09, 2.66e-08, 4.85e-08, 6.66e-08)
# ... and the multi-reference loop ([first, middle, last]) in the same run, for the record (the fused and the loop route gave the
# same five losses):
#     (9.07e-08, 1.15e-07, 1.56e-08, 9.06e-09, 5.69e-08)
# The multi-reference loop runs the same float32 kernels in another summation order (K images per pass, the owner's order in the
# backward), the argument of tests/test_gpu_voxel_loop.py: it is allowed twice the largest of the five.
MULTI_REFERENCE_LOOP_FACTOR = 2.0


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def job_of(plan, directions, pad=0, halo=32, fused=True):
    from event_based_bos_amd import event_plan as EP

    return EP._multiref_job(plan, list(directions), (pad, pad), halo, None, fused, "test")


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("plan_dir", ["first", "middle"])
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("directions", [("middle",), FML, FQML, BMA], ids=["K1", "K3", "K4", "K3-before-after"])
def test_forward_is_the_oracle_per_direction(ebos, directions, pad, plan_dir):
    ev, flow = C.plain_window(), C.flow_u(6.0)
    want = C.cached(("iwes", directions, pad), lambda: C.ref_iwes(ev, flow, directions, pad).numpy())
    plan = C.plan_of(ebos, ev, plan_dir)
    assert plan.ref_fraction == (0.0 if plan_dir == "first" else 0.5) and plan.normalized_t is True
    got = plan.iwe_dense_multi(G(flow, torch.float32), list(directions), pad=(pad, pad), halo=32, fused=True)
    assert got.shape == (len(directions), H + 2 * pad, W + 2 * pad) and got.dtype == torch.float32
    errs = [rel(got[k], want[k]) for k in range(len(directions))]
    print(f"{directions} pad={pad} plan={plan_dir}: IWE rel L2 {errs}")
    assert max(errs) < 1e-4


@pytest.mark.parametrize("case", ["halo32-f32", "halo8-spill", "tile64-halo16", "loop", "none-takes-the-loop"])
def test_forward_routes(ebos, case):
    from event_based_bos_amd import _hip

    fits = _hip.load_library().ebos_iwe_multiref_fits
    tile, halo, amp, fused, directions = C.TILE, 32, 6.0, True, FML
    if case == "halo32-f32":
        assert fits(32, 32, 32, 3) == 1                                               # f32 windows
    elif case == "halo8-spill":
        halo, amp, directions = 8, 12.0, FQML                                         # displacements up to 12 px: beyond the halo
        assert fits(32, 32, 8, 4) == 2
    elif case == "tile64-halo16":
        tile, halo, directions = (64, 64), 16, FQML
    elif case == "loop":
        fused = False
    else:
        tile, halo, fused = (64, 64), 64, None
        assert fits(64, 64, 64, 3) == 0
    ev, flow = C.plain_window(), C.flow_u(amp)
    want = C.cached(("iwes-r", directions, amp), lambda: C.ref_iwes(ev, flow, directions, 0).numpy())
    plan = C.plan_of(ebos, ev, "first", tile)
    job = job_of(plan, directions, 0, halo, fused)
    assert job.halo == halo and job.fused == (fused is True)
    got = plan.iwe_dense_multi(G(flow, torch.float32), list(directions), halo=halo, fused=fused)
    errs = [rel(got[k], want[k]) for k in range(len(directions))]
    print(f"{case}: IWE rel L2 {errs}")
    assert max(errs) < 1e-4
    if case == "halo8-spill":                                                         # the case does leave the 8-pixel halo
        warped = C.O.warp_dense_numpy(ev, flow, "last", True)
        assert (np.abs(warped[:, :2] - ev[:, :2]).max(1) > 9).sum() > 100


AT_LIMIT = {"16x64x32-K2-f64": ((16, 64), 32, ("first", "last"), 2), "16x64x32-K4-f32": ((16, 64), 32, FQML, 1),
            "32x64x48-K1-f64": ((32, 64), 48, ("middle",), 2), "32x64x48-K2-f32": ((32, 64), 48, ("first", "last"), 1)}


@pytest.mark.parametrize("case", list(AT_LIMIT))
def test_forward_with_the_whole_lds(ebos, case):
    """The configurations whose K windows take exactly 160 KiB of dynamic LDS, as float64 and as float32."""
    from event_based_bos_amd import _hip

    tile, halo, directions, kind = AT_LIMIT[case]
    K = len(directions)
    assert _hip.load_library().ebos_iwe_multiref_fits(tile[0], tile[1], halo, K) == kind
    assert K * (tile[0] + 2 * halo) * (tile[1] + 2 * halo) * (8 if kind == 2 else 4) == 160 * 1024
    ev, flow = C.plain_window(), C.flow_u(6.0)
    plan = C.plan_of(ebos, ev, "first", tile)
    job = job_of(plan, directions, 0, halo, True)
    assert job.halo == halo and job.fused
    for pad in (0, 2):
        want = C.cached(("iwes", directions, pad), lambda: C.ref_iwes(ev, flow, directions, pad).numpy())
        got = plan.iwe_dense_multi(G(flow, torch.float32), list(directions), pad=(pad, pad), halo=halo, fused=True)
        errs = [rel(got[k], want[k]) for k in range(K)]
        print(f"{case} pad={pad}: IWE rel L2 {errs}")
        assert got.shape == (K, H + 2 * pad, W + 2 * pad) and bool(torch.isfinite(got).all()) and max(errs) < 1e-4


# ---------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("directions", [("last",), FML, FQML], ids=["K1", "K3", "K4"])
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("omit", [False, True])
def test_backward_is_float64_autograd(ebos, omit, pad, directions):
    flow, ev = C.flow_u(6.0), C.kink_free(directions)
    v_ref, g_ref = C.ref_value_and_grad("kf", ev, flow, directions, "image_variance", omit, pad)
    plan = C.plan_of(ebos, ev)
    f = G(flow, torch.float32).requires_grad_(True)
    v = plan.contrast_dense_multi(f, list(directions), "image_variance", omit, pad=(pad, pad), halo=32, fused=True)
    v.backward()
    print(f"omit={omit} pad={pad} K={len(directions)}: value rel {abs(v.item() - v_ref) / v_ref:.3e}, d_flow rel L2 {rel(f.grad, g_ref):.3e}")
    assert v.dim() == 0 and f.grad.shape == (2, H, W)
    assert abs(v.item() - v_ref) < 1e-5 * v_ref and rel(f.grad, g_ref) < 1e-3


def test_backward_writes_every_cell_and_routes_agree(ebos):
    from event_based_bos_amd import event_plan as EP

    flow, ev = C.flow_u(6.0), C.kink_free(FML)
    _, g_ref = C.ref_value_and_grad("kf", ev, flow, FML, "image_variance", False, 0)
    plan = C.plan_of(ebos, ev)
    f32 = G(flow, torch.float32)
    job = job_of(plan, FML)
    iwes = EP._launch_multiref_fwd(plan, f32, job)
    affine = torch.tensor([[0.37, -0.11], [0.21, 0.05], [-0.4, 0.3]], dtype=torch.float32, device=C.dev())
    outs = [torch.full((2, H, W), fill, dtype=torch.float32, device=C.dev()) for fill in (float("nan"), 7.0)]
    for out in outs:
        assert EP._launch_multiref_bwd(plan, f32, job, iwes, affine, 0, out=out) is out
    assert bool(torch.isfinite(outs[0]).all())                                        # nothing of the NaN fill is left
    assert torch.equal(outs[0], outs[1]) and int(torch.count_nonzero(outs[0])) > 0    # two calls on one set of g_images: the same bits
    empty = plan.pixel_event_counts() == 0
    assert int(torch.count_nonzero(outs[0][:, empty])) == 0                           # exactly zero on pixels without events
    # the loop route on the same upstream: the same sum in another order
    loop = EP._launch_multiref_bwd(plan, f32, job_of(plan, FML, fused=False), iwes, affine, 0)
    print(f"fused against loop, affine upstream: rel L2 {rel(outs[0], loop):.3e}")
    assert rel(outs[0], loop) < 1e-3
    # ... and through the public operator against float64
    grads = []
    for fused in (True, False):
        f = f32.clone().requires_grad_(True)
        plan.contrast_dense_multi(f, list(FML), halo=32, fused=fused).backward()
        grads.append(f.grad)
        assert rel(f.grad, g_ref) < 1e-3
    assert rel(grads[0], grads[1]) < 1e-3
    # a window that leaves whole tiles empty: their pixels are written too, with zeros
    left = ev[ev[:, 1] < 30].copy()
    left[0, 2], left[-1, 2] = 0.0, 1.0
    _, gl_ref = C.ref_value_and_grad("left", left, flow, FML, "image_variance", False, 0)
    lplan = C.plan_of(ebos, left)
    up = torch.full((3,), 1.0 / 3.0, dtype=torch.float32, device=C.dev())
    liwes = EP._launch_multiref_fwd(lplan, f32, job)
    K, h, w = liwes.shape
    lib = ebos.load_library()
    from event_based_bos_amd._hip import check, ptr, stream_ptr
    val = torch.empty(K, dtype=torch.float32, device=C.dev())
    moments = torch.empty((K, 2), dtype=torch.float64, device=C.dev())
    nbytes = int(lib.ebos_cost_scratch_bytes(K))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=C.dev())
    aff = torch.empty((K, 2), dtype=torch.float32, device=C.dev())
    check(lib.ebos_image_variance_f32(ptr(liwes), K, h, w, 0, ptr(val), ptr(moments), ptr(scratch), nbytes, stream_ptr()), "variance")
    check(lib.ebos_image_variance_affine_f32(ptr(moments), ptr(up), K, ptr(aff), stream_ptr()), "affine")
    out = torch.full((2, H, W), float("nan"), dtype=torch.float32, device=C.dev())
    EP._launch_multiref_bwd(lplan, f32, job, liwes, aff, 0, out=out)
    lempty = lplan.pixel_event_counts() == 0
    assert int(lempty.sum()) > 32 * 38 and int(torch.count_nonzero(out[:, lempty])) == 0
    assert bool(torch.isfinite(out).all()) and int(torch.count_nonzero(out[:, :, 32:])) == 0 and rel(out, gl_ref) < 1e-3


def test_hot_pixel_meets_the_gradient_bar(ebos):
    flow = C.flow_u(6.0)
    ev = C.cached("hot", lambda: C.with_hot_pixel(C.kink_free(FML), flow, FML))
    assert len(ev) == N + C.HOT_EXTRA
    v_ref, g_ref = C.ref_value_and_grad("hot", ev, flow, FML)
    plan = C.plan_of(ebos, ev)
    assert int(plan.pixel_event_counts()[C.HOT_PIXEL]) > C.HOT_EXTRA                  # a run the whole wave walks
    f = G(flow, torch.float32).requires_grad_(True)
    v = plan.contrast_dense_multi(f, list(FML), halo=32, fused=True)
    v.backward()
    hot = f.grad[:, C.HOT_PIXEL[0], C.HOT_PIXEL[1]].cpu().numpy()
    want = g_ref[:, C.HOT_PIXEL[0], C.HOT_PIXEL[1]]
    print(f"hot pixel: value rel {abs(v.item() - v_ref) / v_ref:.3e}, d_flow rel L2 {rel(f.grad, g_ref):.3e}, its cell {hot} against {want}")
    assert abs(v.item() - v_ref) < 1e-5 * v_ref and rel(f.grad, g_ref) < 1e-3 and rel(hot, want) < 1e-3


# ---------------------------------------------------------------------------------------------- generic upstream
@pytest.mark.parametrize("fused", [True, False])
def test_generic_upstream_is_float64_autograd(ebos, fused):
    from event_based_bos_amd import ops
    from event_based_bos_amd.event_image_converter import EventImageConverter

    flow, ev = C.flow_u(6.0), C.kink_free(FML)
    plan = C.plan_of(ebos, ev)
    v_ref, g_ref = C.ref_value_and_grad("kf", ev, flow, FML, "gradient_magnitude", True, 2)
    f = G(flow, torch.float32).requires_grad_(True)
    v = plan.contrast_dense_multi(f, list(FML), "gradient_magnitude", True, pad=(2, 2), halo=32, fused=fused)
    v.backward()
    print(f"gradient magnitude (fused={fused}): value rel {abs(v.item() - v_ref) / v_ref:.3e}, d_flow rel L2 {rel(f.grad, g_ref):.3e}")
    assert abs(v.item() - v_ref) < 1e-5 * v_ref and rel(f.grad, g_ref) < 1e-3
    v_ref, g_ref = C.ref_value_and_grad("kf", ev, flow, FML, "image_variance", False, 0, blur=1.0)
    f = G(flow, torch.float32).requires_grad_(True)
    iwes = EventImageConverter._gaussian_blur3(plan.iwe_dense_multi(f, list(FML), halo=32, fused=fused), 1.0)
    v = ops.image_variance(iwes, False).mean()
    v.backward()
    print(f"blurred variance (fused={fused}): value rel {abs(v.item() - v_ref) / v_ref:.3e}, d_flow rel L2 {rel(f.grad, g_ref):.3e}")
    assert abs(v.item() - v_ref) < 1e-5 * v_ref and rel(f.grad, g_ref) < 1e-3


# ---------------------------------------------------------------------------------------------- the solver
def make_solver(ebos, cfg):
    return ebos.solver.collections["contrast_maximization"]((H, W), (H, W), solver_config=cfg)


@pytest.mark.parametrize("case", ["plain", "normalize", "regularised", "blur-two-costs"])
def test_solver_first_loss_and_gradient(ebos, case):
    from event_based_bos_amd import ops

    ev = C.solver_events(FML)
    kw, over = {}, {"fused": case in ("plain", "blur-two-costs")}                     # both routes are covered
    if case == "normalize":
        kw, over = {"normalize": True}, dict(over, normalize=True)
    elif case == "regularised":
        kw = {"w_norm": 0.1, "w_tv": 0.1}
        over = dict(over, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.1, "image_gradient": 0.1})
    elif case == "blur-two-costs":
        kw = {"normalize": True, "blur": 1.0, "weights": {"image_variance": 1.0, "gradient_magnitude": 0.5}}
        over = dict(over, normalize=True, iwe={"blur_sigma": 1}, cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5})
    l_ref, g_ref = C.ref_loss_and_grad(ev, FML, **kw)
    slv = make_solver(ebos, C.solver_config(FML, **over))
    plan = ebos.EventPlan.build(G(ev), (H, W), "first", True, tile=slv.plan_tile(), emit="full")
    theta = G(C.theta_start()).requires_grad_(True)
    loss = slv.objective(plan, ops.upsample_patch_flow(theta, PATCH, PATCH, (H, W)))
    loss.backward()
    print(f"{case}: loss rel {abs(loss.item() - l_ref) / abs(l_ref):.3e}, d_theta rel L2 {rel(theta.grad, g_ref):.3e}")
    assert abs(loss.item() - l_ref) < 1e-5 * abs(l_ref) and rel(theta.grad, g_ref) < 1e-3


def test_solver_adam_loop_follows_the_float64_loop(ebos):
    ev = C.solver_events(FML)
    # the existing single-reference autograd loop against ITS float64 loop, for the record: no block, the same window, the same start
    want1 = np.array(C.ref_adam_losses(ev, ("first",), 5))
    slv = make_solver(ebos, C.solver_config(None))
    slv.previous_best = C.theta_start()
    slv.estimate(ev)
    assert not slv.fused and not slv.graphed and len(slv.history) == 5
    print("single-reference autograd loop, deviation per iteration:", (np.abs(np.array(slv.history) - want1) / np.abs(want1)).tolist())
    want = np.array(C.ref_adam_losses(ev, FML, 5))
    for fused in (True, False):
        slv = make_solver(ebos, C.solver_config(FML, fused=fused))
        slv.previous_best = C.theta_start()
        flow = slv.estimate(ev)
        assert slv.loop_mode == "autograd" and slv.loop_modes == ["autograd"] and not slv.fused and not slv.graphed
        assert flow.shape == (2, H, W) and np.isfinite(flow).all() and len(slv.history) == 5
        dev = np.abs(np.array(slv.history) - want) / np.abs(want)
        print(f"multi-reference loop (fused={fused}), deviation per iteration:", dev.tolist())
        assert want[-1] < want[0] and slv.history[-1] < slv.history[0]                # the loss falls
        assert (dev <= MULTI_REFERENCE_LOOP_FACTOR * max(SINGLE_REFERENCE_LOOP_DEVIATION)).all(), (dev, SINGLE_REFERENCE_LOOP_DEVIATION)


def test_solver_single_direction_scipy_and_pipeline(ebos):
    from event_based_bos_amd.solver import WindowPipeline

    ev = C.solver_events(FML)
    # directions: [<warp_direction>] is the single-reference objective
    single = make_solver(ebos, C.solver_config(None, n_iter=1))
    single.previous_best = C.theta_start()
    single.estimate(ev)
    for fused in (True, False):
        slv = make_solver(ebos, C.solver_config(("first",), n_iter=1, fused=fused))
        slv.previous_best = C.theta_start()
        slv.estimate(ev)
        print(f"directions [first] (fused={fused}): {slv.history[0]} against the single-reference solver's {single.history[0]}")
        assert abs(slv.history[0] - single.history[0]) < 1e-5 * abs(single.history[0])
    # the default tile of a multi-reference solver, and L-BFGS-B from a warm start
    slv = make_solver(ebos, C.solver_config(FML, tile=None, method="L-BFGS-B"))
    assert slv.plan_tile() == (64, 64)
    slv.previous_best = C.theta_start() * 0.2
    slv.estimate(ev)
    print("L-BFGS-B", slv.history[0], "->", float(slv.scipy_result.fun), f"in {len(slv.history)} evaluations")
    assert slv.loop_mode == "autograd" and len(slv.history) >= 2 and float(slv.scipy_result.fun) < slv.history[0]
    with pytest.raises(NotImplementedError, match="multi_reference"):
        WindowPipeline(slv)
