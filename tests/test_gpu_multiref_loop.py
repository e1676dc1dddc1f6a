"""GPU tests of the K-image slab pipeline (``ebos_iwe_dense_slab_multiref_f32``, ``ebos_iwe_dense_tiled_multiref_bwd_f32``), the
``fused="slab"`` route of the plan operators, the native multi-reference Adam loop (``ebos_cmax_multiref_solve_f32`` /
``_gradient_f32``) and the solver's ``multi_reference: {native: true}``.  Yardsticks and windows: tests/_multiref_cases.py (CPU, float64,
torch autograd).  Bars are the project's: IWE relative L2 < 1e-4, values relative < 1e-5, gradients relative L2 < 1e-3; the forward is
compared BIT FOR BIT with the single form on ``dt + shift_k``; the five-iteration bar is taken from the existing autograd loop in the
same run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multiref_cases as C  # noqa: E402
import _multiref_loop_cases as L  # noqa: E402
from _multiref_cases import BMA, FML, FQML, G, H, N, PATCH, W, rel  # noqa: E402

pytestmark = pytest.mark.gpu

# The native loop may lie this many times the largest of the existing autograd loop's five distances from the float64 loop
# (tests/test_gpu_multiref.py uses the rule, tests/test_gpu_voxel_loop.py argues for it: the same float32 kernels' arithmetic in
# another summation order).  The distances themselves are measured in the test, on code this file's subject does not touch.
NATIVE_LOOP_FACTOR = 2.0
# Measured on an MI355X (the test prints them on every run), |loss - loss64| / |loss64| per iteration on solver_events(FML):
#     existing autograd loop (fused: false)   9.07e-08, 1.15e-07, 1.56e-08, 9.06e-09, 5.69e-08
#     native loop                             9.07e-08, 1.15e-07, 1.56e-08, 9.06e-09, 5.69e-08   (the same float32 losses)


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def slab_job(plan, directions, pad=0, halo=32, splits=None):
    from event_based_bos_amd import event_plan as EP

    return EP._multiref_job(plan, list(directions), (pad, pad), halo, splits, "slab", "test")


# ---------------------------------------------------------------------------------------------- 1. forward, bit for bit
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("plan_dir", ["first", "middle"])
@pytest.mark.parametrize("directions,halo", [(("middle",), 8), (FML, 8), (FQML, 8), (BMA, 32)], ids=["K1", "K3", "K4", "K3-before-after"])
def test_forward_has_the_bits_of_the_single_form(ebos, directions, halo, plan_dir, pad, splits):
    """|flow| <= 6 px: with references inside the window |dt_k| <= 1 and halo 8 holds every tap (ceil(6) + 1 = 7); 'before' / 'after' reach
    |dt_k| = 2, 12 px, inside halo 32.  Nothing spills, so both forms sum fixed-point integers and f32 slabs in a fixed order."""
    from event_based_bos_amd import event_plan as EP

    lib = ebos.load_library()
    ev, flow32 = C.plain_window(), G(C.flow_u(6.0), torch.float32)
    plan = C.plan_of(ebos, ev, plan_dir)
    shifts = EP.multi_reference_shifts(plan, list(directions))
    iwes, var, mom, stores, _ = L.slab_multi(lib, plan, shifts, flow32, halo, splits, pad, want_variance=1)
    assert bool(torch.isfinite(iwes).all()) and bool(torch.isfinite(var).all()) and bool(torch.isfinite(mom).all())   # the NaN fill is gone
    assert all(L.guards_intact(s) for s in stores)
    for k, shift in enumerate(shifts):
        want, want_var = L.slab_single(lib, plan, L.padded_dt(plan, shift), flow32, halo, splits, pad, want_variance=1)
        assert torch.equal(iwes[k], want), (directions, k, float((iwes[k] - want).abs().max()))
        assert float(var[k]) == float(want_var[0]) and float(mom[k, 1]) == (H + 2 * pad) * (W + 2 * pad)
    # the public operator returns the same images
    got = plan.iwe_dense_multi(flow32, list(directions), pad=(pad, pad), halo=halo, splits=splits, fused="slab")
    assert torch.equal(got, iwes)


# every triple of the multi-reference slab family (ebos_slab_multiref_config), with the splits the test runs it at
VECTOR_COMBINE_CASES = {"tile32-halo8": ((32, 32), 8, 2), "tile64-halo16": ((64, 64), 16, 1), "tile32-halo32": ((32, 32), 32, 2),
                        "tile64-halo32": ((64, 64), 32, 1)}


def test_the_vector_combine_sweep_is_the_built_set(ebos):
    from event_based_bos_amd import _hip

    assert sorted(t + (hl,) for t, hl, _ in VECTOR_COMBINE_CASES.values()) == sorted(_hip.slab_multiref_configs())


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("tile,halo,splits", list(VECTOR_COMBINE_CASES.values()), ids=list(VECTOR_COMBINE_CASES))
def test_forward_vector_combine_has_the_bits_of_the_single_form(ebos, tile, halo, splits, pad):
    """Image and padding widths that are multiples of 4 take the combine pass that handles four pixels per thread (37 x 70 never
    does): a 37 x 72 window of its own, 8 000 events, |flow| <= 6 px and references inside the window, so nothing leaves halo 8."""
    from event_based_bos_amd import event_plan as EP

    lib = ebos.load_library()
    Hv, Wv = 37, 72
    ev = C.cached(("vec-events",), lambda: C.O.synth_events(8000, Hv, Wv, seed=43, tmin=0.0, tmax=1.0))
    flow32 = torch.from_numpy(np.random.RandomState(23).uniform(-6.0, 6.0, (2, Hv, Wv)).astype(np.float32)).to(C.dev())
    plan = ebos.EventPlan.build(G(ev), (Hv, Wv), "middle", True, tile=tile, emit="full")
    shifts = EP.multi_reference_shifts(plan, list(FQML))
    iwes, var, mom, stores, _ = L.slab_multi(lib, plan, shifts, flow32, halo, splits, pad, want_variance=1, omit=True)
    assert bool(torch.isfinite(iwes).all()) and bool(torch.isfinite(var).all()) and all(L.guards_intact(s) for s in stores)
    for k, shift in enumerate(shifts):
        want, want_var = L.slab_single(lib, plan, L.padded_dt(plan, shift), flow32, halo, splits, pad, want_variance=1, omit=True)
        assert torch.equal(iwes[k], want), (k, float((iwes[k] - want).abs().max()))
        assert float(var[k]) == float(want_var[0]) and float(mom[k, 1]) == (Hv + 2 * pad - 2) * (Wv + 2 * pad - 2)


# ---------------------------------------------------------------------------------------------- 2. forward against float64
@pytest.mark.parametrize("case", ["K3", "K4-pad2", "K3-before-after", "halo8-spill", "tile64-halo16-splits2"])
def test_forward_is_the_oracle_per_direction(ebos, case):
    tile, halo, amp, pad, splits, directions = C.TILE, 32, 6.0, 0, 1, FML
    if case == "K4-pad2":
        pad, directions = 2, FQML
    elif case == "K3-before-after":
        directions = BMA
    elif case == "halo8-spill":
        halo, amp, directions = 8, 12.0, BMA                                          # |dt_k| reaches 2: displacements up to 24 px, far beyond the halo
    elif case == "tile64-halo16-splits2":
        tile, halo, splits, directions = (64, 64), 16, 2, FQML
    ev, flow = C.plain_window(), C.flow_u(amp)
    want = C.cached(("iwes-slab", directions, amp, pad), lambda: C.ref_iwes(ev, flow, directions, pad).numpy())
    plan = C.plan_of(ebos, ev, "first", tile)
    f32 = G(flow, torch.float32)
    got = plan.iwe_dense_multi(f32, list(directions), pad=(pad, pad), halo=halo, splits=splits, fused="slab")
    assert got.shape == (len(directions), H + 2 * pad, W + 2 * pad) and got.dtype == torch.float32
    errs = [rel(got[k], want[k]) for k in range(len(directions))]
    print(f"{case}: IWE rel L2 {errs}")
    assert max(errs) < 1e-4
    if case == "halo8-spill":
        warped = C.O.warp_dense_numpy(ev, flow, "after", True)
        assert (np.abs(warped[:, :2] - ev[:, :2]).max(1) > 9).sum() > 100             # the case does leave the 8-pixel halo
        again = plan.iwe_dense_multi(f32, list(directions), halo=halo, fused="slab")  # the spill sections are zero again
        assert max(rel(again[k], want[k]) for k in range(3)) < 1e-4
    # per-reference variance, boundary omitted or not
    lib = ebos.load_library()
    from event_based_bos_amd import event_plan as EP
    for omit in (False, True):
        _, var, mom, stores, _ = L.slab_multi(lib, plan, EP.multi_reference_shifts(plan, list(directions)), f32, halo, splits, pad, 1, omit)
        assert all(L.guards_intact(s) for s in stores)
        for k in range(len(directions)):
            v_ref = C.O.image_variance(torch.from_numpy(want[k]), omit, "maximize").item()
            assert abs(float(var[k]) - v_ref) < 1e-5 * v_ref, (case, omit, k, float(var[k]), v_ref)


# ---------------------------------------------------------------------------------------------- 3. backward
@pytest.mark.parametrize("directions", [("last",), FML, FQML], ids=["K1", "K3", "K4"])
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("omit", [False, True])
def test_value_and_grad_is_float64_autograd(ebos, omit, pad, directions):
    flow, ev = C.flow_u(6.0), C.kink_free(directions)
    v_ref, g_ref = C.ref_value_and_grad("kf", ev, flow, directions, "image_variance", omit, pad)
    plan = C.plan_of(ebos, ev)
    f32 = G(flow, torch.float32)
    v, g = plan.variance_multi_value_and_grad(f32, list(directions), omit, (pad, pad), 32, None)
    print(f"omit={omit} pad={pad} K={len(directions)}: value rel {abs(v.item() - v_ref) / v_ref:.3e}, d_flow rel L2 {rel(g, g_ref):.3e}")
    assert v.dim() == 0 and g.shape == (2, H, W) and g.dtype == torch.float32
    assert abs(v.item() - v_ref) < 1e-5 * v_ref and rel(g, g_ref) < 1e-3
    # the autograd operator is the same computation
    f = f32.clone().requires_grad_(True)
    va = plan.contrast_dense_multi(f, list(directions), "image_variance", omit, pad=(pad, pad), halo=32, fused="slab")
    va.backward()
    assert va.item() == v.item() and torch.equal(f.grad, g)


def test_hot_pixel_meets_the_gradient_bar(ebos):
    flow = C.flow_u(6.0)
    ev = C.cached("hot", lambda: C.with_hot_pixel(C.kink_free(FML), flow, FML))
    assert len(ev) == N + C.HOT_EXTRA
    v_ref, g_ref = C.ref_value_and_grad("hot", ev, flow, FML)
    plan = C.plan_of(ebos, ev)
    assert int(plan.pixel_event_counts()[C.HOT_PIXEL]) > C.HOT_EXTRA                  # a run the owner's whole wavefront walks
    v, g = plan.variance_multi_value_and_grad(G(flow, torch.float32), list(FML), halo=32)
    hot = g[:, C.HOT_PIXEL[0], C.HOT_PIXEL[1]].cpu().numpy()
    want = g_ref[:, C.HOT_PIXEL[0], C.HOT_PIXEL[1]]
    print(f"hot pixel: value rel {abs(v.item() - v_ref) / v_ref:.3e}, d_flow rel L2 {rel(g, g_ref):.3e}, its cell {hot} against {want}")
    assert abs(v.item() - v_ref) < 1e-5 * v_ref and rel(g, g_ref) < 1e-3 and rel(hot, want) < 1e-3


def test_backward_generic_upstream_every_cell_and_the_same_bits(ebos):
    from event_based_bos_amd import event_plan as EP

    flow, ev = C.flow_u(6.0), C.kink_free(FML)
    plan = C.plan_of(ebos, ev)
    f32 = G(flow, torch.float32)
    # a generic upstream through autograd: within the gradient bar of the existing loop route on the same upstream
    up = torch.from_numpy(np.random.RandomState(5).standard_normal((3, H + 4, W + 4)).astype(np.float32)).to(C.dev())
    grads = []
    for fused in ("slab", False):
        f = f32.clone().requires_grad_(True)
        (plan.iwe_dense_multi(f, list(FML), pad=(2, 2), halo=32, fused=fused) * up).sum().backward()
        grads.append(f.grad)
    print(f"generic upstream, slab against the loop route: rel L2 {rel(grads[0], grads[1]):.3e}")
    assert rel(grads[0], grads[1]) < 1e-3
    # ... and with a halo the displacements leave (8 px against 6 px x |dt_k| <= 1 is inside; 12 px flows are not): global reads of G_k
    wide = G(C.flow_u(12.0), torch.float32)
    grads = []
    for fused, halo in (("slab", 8), (False, 32)):
        f = wide.clone().requires_grad_(True)
        (plan.iwe_dense_multi(f, list(FML), pad=(2, 2), halo=halo, fused=fused) * up).sum().backward()
        grads.append(f.grad)
    print(f"generic upstream beyond the staged halo: rel L2 {rel(grads[0], grads[1]):.3e}")
    assert rel(grads[0], grads[1]) < 1e-3
    # two calls into differently filled outputs: fully written, the same bits, exactly zero on pixels without events
    job = slab_job(plan, FML)
    iwes, _, _ = EP._launch_multiref_slab_fwd(plan, f32, job, 0, False)
    affine = torch.tensor([[0.37, -0.11], [0.21, 0.05], [-0.4, 0.3]], dtype=torch.float32, device=C.dev())
    outs = []
    for fill in (float("nan"), 7.0):
        store, out = L.guarded((2, H, W), fill)
        assert EP._launch_multiref_slab_bwd(plan, f32, job, iwes, affine, 0, out=out) is out
        assert L.guards_intact(store)
        outs.append(out)
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1]) and int(torch.count_nonzero(outs[0])) > 0
    empty = plan.pixel_event_counts() == 0
    assert int(empty.sum()) > 0 and int(torch.count_nonzero(outs[0][:, empty])) == 0
    loop = EP._launch_multiref_bwd(plan, f32, EP._multiref_job(plan, list(FML), (0, 0), 32, None, False, "test"), iwes, affine, 0)
    assert rel(outs[0], loop) < 1e-3
    # a window that leaves whole tiles empty: their pixels are written too, with zeros
    left = ev[ev[:, 1] < 30].copy()
    left[0, 2], left[-1, 2] = 0.0, 1.0
    _, gl_ref = C.ref_value_and_grad("left", left, flow, FML, "image_variance", False, 0)
    lplan = C.plan_of(ebos, left)
    ljob = slab_job(lplan, FML)
    liwes, _, lmom = EP._launch_multiref_slab_fwd(lplan, f32, ljob, 1, False)
    third = torch.full((1,), 1.0 / 3.0, dtype=torch.float32, device=C.dev())
    store, out = L.guarded((2, H, W))
    EP._launch_multiref_slab_bwd(lplan, f32, ljob, liwes, None, 0, lmom, third, out=out)
    lempty = lplan.pixel_event_counts() == 0
    assert L.guards_intact(store) and int(lempty.sum()) > 32 * 38 and int(torch.count_nonzero(out[:, lempty])) == 0
    assert bool(torch.isfinite(out).all()) and int(torch.count_nonzero(out[:, :, 32:])) == 0 and rel(out, gl_ref) < 1e-3
    # addend: added as the gradient is stored, on every cell
    add = torch.from_numpy(np.random.RandomState(6).standard_normal((2, H, W)).astype(np.float32)).to(C.dev())
    with_add = EP._launch_multiref_slab_bwd(lplan, f32, ljob, liwes, None, 0, lmom, third, addend=add)
    assert torch.equal(with_add, out + add)


# ---------------------------------------------------------------------------------------------- 4. the loop, first iteration
def make_solver(ebos, cfg):
    return ebos.solver.collections["contrast_maximization"]((H, W), (H, W), solver_config=cfg)


def make_loop(ebos, directions, capacity=8, **over):
    """(loop, plan) of the block's configuration, from theta_start(): the solver supplies N and the weights, as in ``estimate``."""
    from event_based_bos_amd.solver.multi_reference_loop import MultiReferencePatchLoop

    slv = make_solver(ebos, L.native_config(directions, **over))
    ev = C.solver_events(directions)
    plan = ebos.EventPlan.build(G(ev), (H, W), "first", True, tile=slv.plan_tile(), emit="full")
    norm = slv._multi_reference_norms(plan)["image_variance"]
    loop = MultiReferencePatchLoop(plan, PATCH, PATCH, G(C.theta_start()), list(directions), slv.contrast_terms["image_variance"],
                                   slv.flow_terms.get("flow_norm", 0.0), slv.flow_terms.get("image_gradient", 0.0), slv.omit_boundary,
                                   slv.pad, slv.halo, slv.lr, capacity=capacity, norm=norm)
    return loop, plan


@pytest.mark.parametrize("regularised", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("directions", [FML, BMA], ids=["first-middle-last", "before-middle-after"])
def test_loop_first_loss_and_gradient(ebos, directions, normalize, regularised):
    kw, over = {}, {}
    if normalize:
        kw, over = {"normalize": True}, {"normalize": True}
    if regularised:
        kw = dict(kw, w_norm=0.1, w_tv=0.1)
        over = dict(over, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.1, "image_gradient": 0.1})
    l_ref, g_ref = C.ref_loss_and_grad(C.solver_events(directions), directions, **kw)
    loop, _ = make_loop(ebos, directions, **over)
    assert loop.has_reg == regularised and (loop.norm != 1.0) == normalize
    value, d_theta = loop.value_and_grad(G(C.theta_start()))                          # ebos_cmax_multiref_gradient_f32
    first = float(loop.solve(1)[0])                                                   # losses[0] of ebos_cmax_multiref_solve_f32
    print(f"{directions} normalize={normalize} regularised={regularised}: loss rel {abs(first - l_ref) / abs(l_ref):.3e}, "
          f"d_theta rel L2 {rel(d_theta, g_ref):.3e}")
    assert abs(first - l_ref) < 1e-5 * abs(l_ref) and abs(float(value) - l_ref) < 1e-5 * abs(l_ref)
    assert rel(d_theta, g_ref) < 1e-3
    assert torch.equal(loop.d_theta, d_theta)                                         # the step's gradient is the gradient entry's


# ---------------------------------------------------------------------------------------------- 5. the loop, five iterations
def test_loop_follows_the_float64_loop_and_repeats_its_bits(ebos):
    ev = C.solver_events(FML)
    want = np.array(C.ref_adam_losses(ev, FML, 5))
    # the EXISTING multi-reference autograd loop (fused: false, no native) in this run: its distances set the bar
    slv = make_solver(ebos, C.solver_config(FML, fused=False))
    slv.previous_best = C.theta_start()
    slv.estimate(ev)
    assert slv.loop_mode == "autograd" and len(slv.history) == 5
    dev_autograd = np.abs(np.array(slv.history) - want) / np.abs(want)
    loop, _ = make_loop(ebos, FML)
    losses = loop.solve(5).cpu().numpy().astype(np.float64)
    dev_native = np.abs(losses - want) / np.abs(want)
    print("existing autograd multi-reference loop, deviation per iteration:", dev_autograd.tolist())
    print("native multi-reference loop, deviation per iteration:           ", dev_native.tolist())
    assert want[-1] < want[0] and losses[-1] < losses[0]                              # the loss falls
    assert (dev_native <= NATIVE_LOOP_FACTOR * dev_autograd.max()).all(), (dev_native, dev_autograd)
    # a second loop: the same bits in theta and losses; n_iter 2 + 3 continues to the bits of 5
    again, _ = make_loop(ebos, FML)
    assert torch.equal(again.solve(5), loop.losses[:5]) and torch.equal(again.theta, loop.theta)
    split, _ = make_loop(ebos, FML)
    split.solve(2)
    split.solve(3)
    assert split.t == 5 and int(split.step[0]) == 5
    assert torch.equal(split.losses[:5], loop.losses[:5]) and torch.equal(split.theta, loop.theta)
    assert torch.equal(split.exp_avg, loop.exp_avg) and torch.equal(split.exp_avg_sq, loop.exp_avg_sq)
    with pytest.raises(ValueError, match="capacity"):
        split.solve(4)


# ---------------------------------------------------------------------------------------------- 6. the solver
def test_solver_runs_the_native_loop(ebos):
    from event_based_bos_amd import ops

    ev = C.solver_events(FML)
    slv = make_solver(ebos, L.native_config(FML))
    slv.previous_best = C.theta_start()
    flow = slv.estimate(ev)
    assert slv.loop_mode == "native" and slv.loop_modes == ["native"] and slv.fused and not slv.graphed
    loop, _ = make_loop(ebos, FML)
    loop.solve(5)
    want_flow = ops.upsample_patch_flow(loop.theta, PATCH, PATCH, (H, W)).cpu().numpy()
    assert flow.shape == (2, H, W) and np.array_equal(np.asarray(flow, dtype=np.float32), want_flow.astype(np.float32))
    assert slv.history == loop.losses[:5].cpu().tolist() and torch.equal(slv.patch_flow, loop.theta)
    # L-BFGS-B through the loop's value_and_grad, from a warm start
    lb = make_solver(ebos, L.native_config(FML, method="L-BFGS-B"))
    lb.previous_best = C.theta_start() * 0.2
    lb.estimate(ev)
    probe, _ = make_loop(ebos, FML)
    value, _ = probe.value_and_grad(G(C.theta_start() * 0.2))
    print("L-BFGS-B (native)", lb.history[0], "->", float(lb.scipy_result.fun), f"in {len(lb.history)} evaluations")
    assert lb.loop_mode == "native" and lb.fused and lb.history[0] == float(value)
    assert len(lb.history) >= 2 and float(lb.scipy_result.fun) < lb.history[0]
