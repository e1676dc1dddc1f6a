"""GPU tests of the contrast's Hessian-vector product: the tangent forward (``ebos_iwe_dense_tangent_tiled_f32``), the owner product
(``ebos_iwe_dense_hvp_owner_bwd_f32``), ``EventPlan.iwe_dense_jvp`` / ``contrast_dense_hvp`` and the solver's Newton-CG / trust-ncg /
trust-krylov.  Yardsticks and windows: tests/_hvp_cases.py (CPU, float64, ``torch.autograd.functional.hvp``).  Bars are the project's:
IWE relative L2 < 1e-4, values relative < 1e-5, gradients and products relative L2 < 1e-3.

The float32 CPU evaluation of the same formula lies 1.3e-6 (product) and 1.6e-6 (gradient) from the float64 yardstick
(tests/test_hvp.py::test_closed_form_in_float32_is_close); every test prints what the kernels give."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hvp_cases as C  # noqa: E402
from _hvp_cases import G, H, PATCH, W, rel  # noqa: E402

pytestmark = pytest.mark.gpu

HESSP_METHODS = ("Newton-CG", "trust-ncg", "trust-krylov")


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def plan_of(ebos, ev, tile=C.TILE):
    return C.M.plan_of(ebos, ev, "first", tile)


def make_solver(ebos, cfg):
    return ebos.solver.ContrastMaximization((H, W), (H, W), solver_config=cfg)


def operands(amp=6.0):
    return G(C.flow_u(amp), torch.float32), G(C.direction_v(), torch.float32)


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("case", ["amp6-halo16", "amp12-halo8-spill"])
def test_jvp_images_are_the_float64_images(ebos, case, pad):
    from event_based_bos_amd import _hip

    amp, halo = (6.0, 16) if case == "amp6-halo16" else (12.0, 8)
    ev = C.kink_free(amp)
    want_iwe, want_tangent = C.ref_images(("kf", amp), ev, C.flow_u(amp), C.direction_v(), pad)
    plan = plan_of(ebos, ev)
    flow, v = operands(amp)
    assert _hip.load_library().ebos_iwe_multiref_fits(32, 32, halo, 2) == 2           # float64 windows, with and without the IWE
    iwe, tangent = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=halo)
    assert iwe.shape == tangent.shape == (H + 2 * pad, W + 2 * pad) and iwe.dtype == tangent.dtype == torch.float32
    none, alone = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=halo, with_iwe=False)
    _, atomic = plan.iwe_dense_jvp(flow, v, pad=(pad, pad), halo=halo, splits=2)      # the atomic flush, two work items per tile
    errs = (rel(iwe, want_iwe), rel(tangent, want_tangent), rel(alone, want_tangent), rel(atomic, want_tangent))
    print(f"{case} pad={pad}: IWE rel L2 {errs[0]:.3e}, tangent {errs[1]:.3e}, tangent alone {errs[2]:.3e}, atomic flush {errs[3]:.3e}; "
          f"with / without the IWE bit-identical: {torch.equal(tangent, alone)}, rel L2 {rel(alone, tangent):.3e}")
    assert none is None and max(errs) < 1e-4
    # With and without the IWE: the same float64 windows, summed by the combine pass in the same order -- the same bits where nothing
    # spills; the spill path's float atomics (and the atomic flush) agree within the bar.
    assert rel(alone, tangent) < 1e-4 and rel(atomic, tangent) < 1e-4
    if not case.endswith("spill"):
        assert torch.equal(tangent, alone)
    if case.endswith("spill"):                                                         # the case does leave the 8-pixel halo
        warped = C.O.warp_dense_numpy(ev, C.flow_u(amp), "first", True)
        assert (np.abs(warped[:, :2] - ev[:, :2]).max(1) > 9).sum() > 100


def test_jvp_accumulates_into_zero_filled_images_and_nowhere_else(ebos):
    """The entry adds into caller-zeroed images: the same images inside a larger buffer, whose guard cells it leaves alone."""
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    ev = C.kink_free()
    plan = plan_of(ebos, ev)
    flow, v = operands()
    iwe, tangent = plan.iwe_dense_jvp(flow, v, pad=(2, 2), halo=16)
    h, w = H + 4, W + 4
    guard = 4096
    big = torch.full((guard + 2 * h * w + guard,), float("nan"), dtype=torch.float32, device=C.dev())
    big[guard:guard + 2 * h * w] = 0.0
    t_at, i_at = big[guard:guard + h * w], big[guard + h * w:guard + 2 * h * w]
    lib = ebos.load_library()
    check(lib.ebos_iwe_dense_tangent_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow), ptr(v), H, W,
                                               32, 32, 16, 1, 2, 2, ptr(i_at), ptr(t_at), stream_ptr()), "tangent")
    torch.cuda.synchronize()
    assert bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[-guard:]).all())
    print(f"in a guarded buffer: IWE rel L2 {rel(i_at.reshape(h, w), iwe):.3e} (bits equal: {torch.equal(i_at.reshape(h, w), iwe)}), "
          f"tangent {rel(t_at.reshape(h, w), tangent):.3e} (bits equal: {torch.equal(t_at.reshape(h, w), tangent)})")
    assert rel(i_at.reshape(h, w), iwe) < 1e-6 and rel(t_at.reshape(h, w), tangent) < 1e-4


# ---------------------------------------------------------------------------------------------- product
def check_product(what, got, want):
    value, d_flow, hv = got
    errs = (abs(float(value) - want[0]) / abs(want[0]), rel(d_flow, want[1]), rel(hv, want[2]))
    print(f"{what}: value rel {errs[0]:.3e}, d_flow rel L2 {errs[1]:.3e}, hv rel L2 {errs[2]:.3e}")
    assert value.dim() == 0 and d_flow.shape == hv.shape == (2, H, W) and d_flow.dtype == hv.dtype == torch.float32
    assert errs[0] < 1e-5 and errs[1] < 1e-3 and errs[2] < 1e-3
    return errs


@pytest.mark.parametrize("blur", [0.0, 1.0])
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("omit", [False, True])
@pytest.mark.parametrize("cost", ["image_variance", "gradient_magnitude"])
def test_product_is_float64_autograd(ebos, cost, omit, pad, blur):
    ev = C.kink_free()
    want = C.ref_hvp("kf", ev, C.flow_u(), C.direction_v(), cost, omit, pad, blur)
    flow, v = operands()
    got = plan_of(ebos, ev).contrast_dense_hvp(flow, v, cost, omit, blur, pad=(pad, pad))
    check_product(f"{cost} omit={omit} pad={pad} blur={blur}", got[:3], want)


def test_product_of_two_weighted_costs(ebos):
    ev = C.kink_free()
    flow, v = operands()
    for blur in (0.0, 1.0):
        want = C.ref_hvp("kf", ev, C.flow_u(), C.direction_v(), C.TWO_COSTS, False, 0, blur)
        got = plan_of(ebos, ev).contrast_dense_hvp(flow, v, dict(C.TWO_COSTS), blur_sigma=blur)
        check_product(f"variance + 0.5 gradient magnitude, blur={blur}", got[:3], want)
    # a weighted single cost takes the affine route with its weight
    want = C.ref_hvp("kf", ev, C.flow_u(), C.direction_v(), {"image_variance": 0.25}, True, 2, 0.0)
    got = plan_of(ebos, ev).contrast_dense_hvp(flow, v, {"image_variance": 0.25}, True, pad=(2, 2))
    check_product("0.25 variance, omit, pad 2", got[:3], want)


def test_product_on_a_hot_pixel(ebos):
    """3000 events on one source pixel, times shuffled: the whole wave walks the run."""
    ev = C.with_hot_pixel()
    plan = plan_of(ebos, ev)
    assert int(plan.pixel_event_counts().max()) >= C.M.HOT_EXTRA
    flow, v = operands()
    for cost in ("image_variance", "gradient_magnitude"):
        want = C.ref_hvp("hot", ev, C.flow_u(), C.direction_v(), cost, False, 0, 0.0)
        check_product(f"hot pixel, {cost}", plan.contrast_dense_hvp(flow, v, cost)[:3], want)


STATE_CASES = (("image_variance", 0.0), (dict(C.TWO_COSTS), 1.0))


def test_product_with_a_reused_state_is_bit_identical(ebos):
    """``hv`` from a reused ``state`` equals the product computed without one, bit for bit; so do ten repeated products.

    The owner kernel gives the same bits for the same upstream images, and the tangent image repeats its bits because the operators
    take the slab route: float64 windows per tile, summed per cell in tile order.  (On the atomic flush the same window's tangent
    took 3 - 12 distinct bit patterns in 40 calls on an MI355X -- at the corners where four 32 x 32 tiles meet, three or more sums
    meet in float32 atomics -- and ``hv`` with and without a state agreed bit for bit in 6 of 40 pairs.)"""
    plan = plan_of(ebos, C.kink_free())
    flow, v = operands()
    equal = []
    for cost, blur in STATE_CASES:
        value, d_flow, hv, state = plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur)
        hv2 = plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur, state=state)[2]
        equal.append(torch.equal(hv2, hv))
        again = [torch.equal(plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur)[2], hv) for _ in range(10)]
        print(f"{cost} blur={blur}: hv with the reused state against without, rel L2 {rel(hv2, hv):.3e}, bits equal: {equal[-1]}; "
              f"ten more products without a state, bits equal: {sum(again)} of 10")
        equal += again
    assert all(equal)


def test_product_with_a_reused_state_and_two_owner_calls(ebos):
    from event_based_bos_amd import event_plan as EP

    ev = C.kink_free()
    plan = plan_of(ebos, ev)
    flow, v = operands()
    w = G(C.direction_v(92), torch.float32)
    for cost, blur in STATE_CASES:
        value, d_flow, hv, state = plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur)
        value2, d_flow2, hv2, state2 = plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur, state=state)
        assert state2 is state and value2 is value and d_flow2 is d_flow              # what depends on the flow alone is kept
        print(f"{cost} blur={blur}: hv with the reused state against without, rel L2 {rel(hv2, hv):.3e}")
        assert rel(hv2, hv) < 1e-3
        # another direction at the same flow, against the yardstick; and the symmetry of the Hessian
        hw = plan.contrast_dense_hvp(flow, w, cost, blur_sigma=blur, state=state)[2]
        want = C.ref_hvp("kf", ev, C.flow_u(), C.direction_v(92), cost, False, 0, blur)
        a, b = float((w.double() * hv.double()).sum()), float((v.double() * hw.double()).sum())
        print(f"    second direction: hv rel L2 {rel(hw, want[2]):.3e}; <w, Hv> = {a:.6e}, <v, Hw> = {b:.6e}, relative difference {abs(a - b) / abs(a):.3e}")
        assert rel(hw, want[2]) < 1e-3 and abs(a - b) < 1e-3 * abs(a)
        with pytest.raises(ValueError, match="other options"):
            plan.contrast_dense_hvp(flow, v, cost, blur_sigma=blur, pad=(2, 2), state=state)
    # the owner entry twice on one pair of upstream images: no atomics, the same bits; nothing of a NaN fill is left
    iwe, tangent = plan.iwe_dense_jvp(flow, v, halo=16)
    affine = torch.tensor([0.37, -0.11, 0.21, 0.05], dtype=torch.float32, device=C.dev())
    outs = [EP._launch_hvp_owner(plan, flow, v, (0, 0), iwe, tangent, affine, 0, True) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and int(torch.count_nonzero(outs[0][1])) > 0
    empty = plan.pixel_event_counts() == 0
    assert int(torch.count_nonzero(outs[0][1][:, empty])) == 0 and int(torch.count_nonzero(outs[0][0][:, empty])) == 0


def test_product_of_an_empty_plan_is_zero(ebos):
    """n == 0: the owner entry still writes every cell, with zeros -- into NaN-filled outputs here."""
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    dev = C.dev()
    none = torch.zeros(0, dtype=torch.float32, device=dev)
    keys = 2 * 3 * 32 * 32
    plan = ebos.EventPlan(none, none, none, none, (H, W), 0, 0, tile=(32, 32), key_offsets=torch.zeros(keys + 1, dtype=torch.int32, device=dev))
    flow, v = operands()
    iwe, tangent = plan.iwe_dense_jvp(flow, v)
    assert int(torch.count_nonzero(iwe)) == 0 and int(torch.count_nonzero(tangent)) == 0
    outs = [torch.full((2, H, W), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    check(ebos.load_library().ebos_iwe_dense_hvp_owner_bwd_f32(None, None, None, ptr(plan.key_offsets), 0, ptr(flow), ptr(v), H, W, 32, 32, 0, 0,
                                                               ptr(iwe), ptr(tangent), None, 0, ptr(outs[0]), ptr(outs[1]), stream_ptr()),
          "owner")
    assert int(torch.count_nonzero(outs[0])) == 0 and int(torch.count_nonzero(outs[1])) == 0      # (NaN counts as non-zero)
    value, d_flow, hv, _ = plan.contrast_dense_hvp(flow, v)
    assert float(value) == 0.0 and int(torch.count_nonzero(d_flow)) == 0 and int(torch.count_nonzero(hv)) == 0


# ---------------------------------------------------------------------------------------------- solver
SOLVER_CASES = {
    "plain": ({}, {}),
    "regularised": ({"w_norm": 0.1, "w_tv": 0.1}, {"cost_with_weight": {"image_variance": 1.0, "flow_norm": 0.1, "image_gradient": 0.1}}),
    "blur-two-costs": ({"blur": 1.0, "weights": dict(C.TWO_COSTS)}, {"iwe": {"blur_sigma": 1}, "cost_with_weight": dict(C.TWO_COSTS)}),
}


@pytest.mark.parametrize("case", list(SOLVER_CASES))
def test_solver_hessp_is_the_float64_product(ebos, case):
    kw, over = SOLVER_CASES[case]
    ev = C.solver_events()
    gh, gw = C.O.patch_grid_shape((H, W), PATCH, PATCH)
    p = np.random.RandomState(93).standard_normal((2, gh, gw))
    l_ref, g_ref, hp_ref = C.ref_loss_hvp(ev, p, **kw)
    slv = make_solver(ebos, C.solver_config("Newton-CG", **over))
    plan = slv._build_plan(ev)
    assert not plan.lean and tuple(plan.tile) == C.TILE
    value_and_grad, hessp = slv._hessp_objective(plan, PATCH, PATCH, None)
    theta = torch.from_numpy(C.theta_start()).double()
    loss, grad = value_and_grad(theta)
    hp = hessp(theta, torch.from_numpy(p))
    errs = (abs(float(loss) - l_ref) / abs(l_ref), rel(grad, g_ref), rel(hp, hp_ref))
    print(f"{case}: loss rel {errs[0]:.3e}, d_theta rel L2 {errs[1]:.3e}, H p rel L2 {errs[2]:.3e}")
    assert slv.hessp_calls == 1 and errs[0] < 1e-5 and errs[1] < 1e-3 and errs[2] < 1e-3
    # a product asked at another theta evaluates there first
    hp2 = hessp(theta * 0.5, torch.from_numpy(p))
    assert slv.hessp_calls == 2 and rel(hp2, hp) > 1e-2


def float64_run(method, scale, n_iter=5):
    """scipy on the float64 loss alone: (final loss, products)."""
    import scipy.optimize as sopt

    def make():
        ev, shape, calls = C.solver_events(), C.theta_start().shape, [0]

        def fun(x):
            th = torch.from_numpy(x.reshape(shape)).requires_grad_(True)
            loss = C.ref_loss(th, ev)
            (g,) = torch.autograd.grad(loss, th)
            return loss.item(), g.numpy().reshape(-1)

        def hessp(x, q):
            calls[0] += 1
            fn = lambda t: C.ref_loss(t, ev)   # noqa: E731
            return torch.autograd.functional.hvp(fn, torch.from_numpy(x.reshape(shape)), torch.from_numpy(q.reshape(shape)))[1].numpy().reshape(-1)

        res = sopt.minimize(fun, (scale * C.theta_start()).astype(np.float64).reshape(-1), jac=True, hessp=hessp, method=method,
                            options={"maxiter": n_iter})
        return float(res.fun), calls[0]
    return C.cached(("f64-run", method, scale, n_iter), make)


@pytest.mark.parametrize("scale", [1.0, 0.2])
@pytest.mark.parametrize("method", HESSP_METHODS)
def test_solver_methods_descend(ebos, method, scale):
    ev = C.solver_events()
    slv = make_solver(ebos, C.solver_config(method))
    slv.previous_best = scale * C.theta_start()
    flow = slv.estimate(ev)
    with torch.no_grad():
        start = C.ref_loss(torch.from_numpy(scale * C.theta_start()).double(), ev).item()
        final = C.ref_loss(slv.patch_flow.detach().cpu().double(), ev).item()
    f64_final, f64_calls = float64_run(method, scale)
    print(f"{method} from {scale} theta_start: {slv.history[0]:.5f} -> {float(slv.scipy_result.fun):.5f} in {len(slv.history)} evaluations and "
          f"{slv.hessp_calls} products; float64 loss at the result {final:.5f} (start {start:.5f}); the float64 run ends at {f64_final:.5f} "
          f"after {f64_calls} products: deviation {abs(final - f64_final) / abs(f64_final):.3e}")
    assert slv.loop_mode == "hessp" and slv.loop_modes == ["hessp"] and not slv.fused and not slv.graphed
    assert flow.shape == (2, H, W) and np.isfinite(flow).all()
    assert slv.hessp_calls >= 1 and float(slv.scipy_result.fun) < slv.history[0] and final < start


@pytest.mark.parametrize("case", ["pyramid", "masked"])
def test_solver_pyramid_and_mask(ebos, case):
    ev = C.solver_events()
    if case == "pyramid":
        over = {"patch": {"size": list(PATCH), "sliding_window": list(PATCH), "pyramid": {"coarsest": 16, "finest": 8}}}
    else:
        over = {"patch": {"size": list(PATCH), "sliding_window": list(PATCH), "do_event_thresholding": True, "event_thres": 1000}}
        # (the three full rows of patches hold 1239 - 1347 events each, the patches of the one-pixel row below them 93 - 117)
    slv = make_solver(ebos, C.solver_config("Newton-CG", n_iter=6, iwe={"blur_sigma": 1}, **over))
    if case == "masked":
        slv.previous_best = 0.2 * C.theta_start()
    else:   # (the coarsest grid's own shape)
        gh, gw = C.O.patch_grid_shape((H, W), (16, 16), (16, 16))
        slv.previous_best = np.full((2, gh, gw), 0.3, dtype=np.float32)
    flow = slv.estimate(ev)
    print(f"{case}: {slv.history[0]:.5f} -> {min(slv.history):.5f}, {len(slv.history)} evaluations, {slv.hessp_calls} products, scales {slv.loop_modes}")
    assert np.isfinite(flow).all() and slv.hessp_calls >= 1 and min(slv.history) < slv.history[0]
    if case == "pyramid":
        assert slv.loop_modes == ["hessp", "hessp"] and len(slv.patch_flow_per_scale) == 2
    else:
        mask = slv.patch_mask(slv._build_plan(ev), PATCH, PATCH)
        assert 0 < int(mask.sum()) < mask.numel()                                     # some patches are estimated, some are not ...
        assert int(torch.count_nonzero(slv.patch_flow[:, mask == 0])) == 0            # ... and those keep zero flow


def test_newton_cg_yaml_runs_one_estimate(ebos):
    import yaml

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "cmax_newton_cg.yaml")))["solver"]
    assert cfg["optimizer"]["method"] == "Newton-CG"
    cfg["tile"] = list(C.TILE)
    cfg["optimizer"]["n_iter"] = 3
    slv = make_solver(ebos, cfg)
    slv.previous_best = None
    gh, gw = C.O.patch_grid_shape((H, W), slv.patch_size, slv.sliding_window)
    slv.previous_best = np.full((2, gh, gw), 0.5, dtype=np.float32)
    flow = slv.estimate(C.solver_events())
    print(f"configs/cmax_newton_cg.yaml at {H} x {W}: {slv.history[0]:.5f} -> {min(slv.history):.5f}, {slv.hessp_calls} products")
    assert slv.loop_mode == "hessp" and flow.shape == (2, H, W) and np.isfinite(flow).all() and np.isfinite(slv.history).all()
