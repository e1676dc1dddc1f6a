"""The contrast-maximisation solver behind the reference's solver registry ("next" row f.1 of SURVEY 8).
CPU part: registry, YAML keys, error behaviour.  GPU part: the solver recovers a known motion, and its
Adam trajectory matches the same loop driven by the CPU oracle (fp64)."""
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import ebos_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_cfg():
    return yaml.safe_load(open(os.path.join(ROOT, "configs", "cmax_hot_plate1.yaml")))


def moving_points(h, w, n_points, per_point, v, seed=0):
    """Events of points translating with velocity v (px per window): the contrast peaks at flow == v."""
    rs = np.random.RandomState(seed)
    p0 = np.stack([rs.uniform(8, h - 16, n_points), rs.uniform(8, w - 16, n_points)], 1)
    t = rs.uniform(0, 1, (n_points, per_point))
    x = np.rint(p0[:, None, 0] + t * v[0]).reshape(-1)
    y = np.rint(p0[:, None, 1] + t * v[1]).reshape(-1)
    ev = np.stack([x, y, t.reshape(-1) * 0.02 + 10.0, rs.randint(0, 2, x.size)], 1)
    ev = ev[(ev[:, 0] >= 0) & (ev[:, 0] < h) & (ev[:, 1] >= 0) & (ev[:, 1] < w)]
    return ev[np.argsort(ev[:, 2], kind="stable")]


def test_registry_and_config_keys():
    import event_based_bos_amd as ebos

    cfg = load_cfg()
    assert set(cfg) >= {"is_dnn", "data", "common_params", "solver"}
    cls = ebos.solver.collections[cfg["solver"]["method"]]
    s = cls((260, 346), (260, 346), calibration_parameter=None, solver_config=cfg["solver"], visualize_module=None)
    assert isinstance(s, ebos.solver.SolverBase)
    assert s.contrast_terms == {"image_variance": 1.0} and s.flow_terms == {"flow_norm": 0.001}
    assert s.orig_warper.normalize_t and s.orig_imager.image_size == (260, 346)
    assert ebos.solver.patch_grid_shape((720, 1280), (24, 32), (24, 32)) == (30, 40)
    with pytest.raises(ValueError):
        cls((8, 8), (8, 8), solver_config={"cost_with_weight": {"flow_norm": 1.0}})
    with pytest.raises(KeyError):
        cls((8, 8), (8, 8), solver_config={"cost_with_weight": {"image_variance": 1.0, "nope": 1.0}})
    assert cls((8, 8), (8, 8), solver_config={"iwe": {"blur_sigma": 1}}).blur_sigma == 1.0
    with pytest.raises(NotImplementedError):
        cls((8, 8), (8, 8), solver_config={"iwe": {"method": "count"}})


def test_pyramid_schedule_follows_reference():
    """patch.pyramid {64, 8}: scales 1..4 with square patches 64, 32, 16, 8 (src/solver/patch_eklt_pyramid2.py:55-83)
    and n_iter // (finest_scale - scale + 1) iterations each (:260)."""
    import event_based_bos_amd as ebos

    cls = ebos.solver.collections["contrast_maximization"]
    s = cls((720, 1280), (720, 1280), solver_config={"patch": {"pyramid": {"coarsest": 64, "finest": 8}},
                                                      "optimizer": {"method": "Adam", "n_iter": 600}})
    assert s.pyramid_scales() == [((64, 64), (64, 64), 120), ((32, 32), (32, 32), 150), ((16, 16), (16, 16), 200),
                                  ((8, 8), (8, 8), 300)]
    s1 = cls((96, 128), (96, 128), solver_config={"patch": {"size": [24, 32]}, "optimizer": {"n_iter": 7}})
    assert s1.pyramid_scales() == [((24, 32), (24, 32), 7)]
    with pytest.raises(ValueError):
        cls((8, 8), (8, 8), solver_config={"patch": {"pyramid": {"coarsest": 4, "finest": 8}}})


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer,patch", [
    ({"method": "Adam", "n_iter": 120, "parameters": {"lr": 0.5}}, {"pyramid": {"coarsest": 32, "finest": 16}}),
    ({"method": "L-BFGS-B", "n_iter": 60}, {"size": [48, 64], "sliding_window": [48, 64]}),
    ({"method": "BFGS", "n_iter": 60}, {"size": [48, 64], "sliding_window": [48, 64]}),
    ({"method": "CG", "n_iter": 60}, {"size": [24, 32], "sliding_window": [24, 32]}),
])
def test_solver_pyramid_and_scipy_optimisers(optimizer, patch):
    """Coarse-to-fine patch pyramid and the scipy first-order optimisers, on the blurred-IWE objective: both must
    raise the contrast of the un-blurred IWE and land near the true translation."""
    import event_based_bos_amd as ebos

    h, w = 96, 128
    v = np.array([5.0, -3.0])
    ev = moving_points(h, w, 600, 40, v, seed=3)
    cfg = load_cfg()["solver"]
    cfg.update(patch=patch, optimizer=optimizer, cost_with_weight={"image_variance": 1.0},
               iwe={"method": "bilinear_vote", "blur_sigma": 1})
    s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    if optimizer["method"] != "Adam":
        # line-search methods must not start on the kink of the objective: with integer sensor coordinates and zero
        # flow every event sits exactly on a pixel centre, where the bilinear vote is only one-sided differentiable
        gh, gw = ebos.solver.patch_grid_shape((h, w), patch["size"], patch["sliding_window"])
        s.set_previous_frame_best_estimation(np.full((2, gh, gw), 0.25))
    flow = s.estimate(ev)
    assert flow.shape == (2, h, w)
    assert min(s.history) < s.history[0] * 1.2, (s.history[0], min(s.history))
    med = np.median(flow[:, 16:-16, 16:-16].reshape(2, -1), axis=1)
    # (Adam at lr 0.5 px per step does not settle: the median lands within ~1 px of the truth, which way depends on the last bits)
    assert np.all(np.abs(med - v) < 1.3), med
    if "pyramid" in patch:
        assert [tuple(t.shape) for t in s.patch_flow_per_scale] == [(2, 3, 4), (2, 6, 8)]
        assert len(s.history) == 120 // 3 + 120 // 2


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [{"image_variance": 1.0}, {"image_variance": 2.0, "flow_norm": 0.01, "image_gradient": 0.05},
                                   {"gradient_magnitude": 3.0, "flow_norm": 0.02}, {"gradient_magnitude": 1.0}])
def test_fused_loop_follows_the_autograd_loop(terms):
    """The fixed kernel pipeline (solver/fused_loop.py) and the autograd loop minimise the same objective with the same
    Adam: loss histories agree to 1e-4 relative and the patch flows to 2e-3 px over 40 iterations (both f32)."""
    import event_based_bos_amd as ebos

    h, w = 96, 128
    ev = moving_points(h, w, 500, 40, np.array([4.0, -2.5]), seed=5)
    out = {}
    for fused in (True, False):
        cfg = load_cfg()["solver"]
        cfg.update(patch={"size": [24, 32], "sliding_window": [24, 32]}, cost_with_weight=terms,
                   iwe={"method": "bilinear_vote", "blur_sigma": 0},
                   optimizer={"method": "Adam", "n_iter": 40, "parameters": {"lr": 0.2}, "graph": True, "fused": fused})
        s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
        s.estimate(ev)
        assert s.fused == fused and s.graphed == (not fused)
        if fused:  # either contrast as ONE resident launch (moving points at 4 px: the windows stay inside its LDS regions)
            assert s.loop_mode == "resident", s.loop_mode
        out[fused] = (np.array(s.history), s.patch_flow.cpu().numpy())
    rel_dev = np.abs(out[True][0] - out[False][0]) / np.abs(out[False][0])
    print("max relative deviation per iteration", np.round(rel_dev, 6), "flow", np.abs(out[True][1] - out[False][1]).max())
    assert rel_dev[:10].max() < 1e-4 and rel_dev.max() < 2e-2
    assert np.abs(out[True][1] - out[False][1]).max() < 0.25


@pytest.mark.gpu
def test_fused_loop_run_modes_agree():
    """FusedPatchLoop: the native loop (ebos_cmax_patch_solve_f32 once), one such call per iteration (``native=False``: the same
    launches with the same arguments) and the resident launch (ebos_cmax_patch_solve_resident_f32) run the same arithmetic in the
    same order: the losses of 30 iterations are the same bit for bit; a loop can be continued in another mode (10 + 20 steps)."""
    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = 96, 128
    ev = moving_points(h, w, 500, 40, np.array([4.0, -2.5]), seed=6)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto")
    hist = {}
    for mode in ("native", "resident", "python", "split"):
        # halo "auto" (the solver's default): the resident kernel always sizes its windows at run time, and the backward scatter's
        # fixed-point unit follows max |upstream| over the staged WINDOW -- against a built halo it agrees to ~1e-6, not bit for bit
        loop = FusedPatchLoop(plan, (24, 32), (24, 32), torch.zeros((2, 4, 4)), 1.0, 0.01, 0.02, halo="auto", lr=0.1, capacity=30)
        assert loop.resident_supported(), ebos.load_library().ebos_last_error()
        if mode == "split":    # 10 iterations of the resident launch (the default mode), continued with one host call per iteration
            first = loop.run(10).cpu().numpy()
            assert loop.last_run_mode == "resident"
            hist[mode] = np.concatenate([first, loop.run(20, native=False).cpu().numpy()])
        elif mode == "resident":
            hist[mode] = loop.run(30, resident=True).cpu().numpy()
            assert loop.last_run_mode == "resident" and loop.resident_status == 0
        else:
            hist[mode] = loop.run(30, native=mode == "native", resident=False).cpu().numpy()
            assert loop.last_run_mode == "pipeline"
        assert loop.t == 30 and int(loop.step.item()) == 30
    np.testing.assert_array_equal(hist["python"], hist["native"])
    np.testing.assert_array_equal(hist["split"], hist["native"])
    np.testing.assert_array_equal(hist["resident"], hist["native"])   # the resident launch follows the pipeline bit for bit
    # EBOS_RESIDENT=0 turns the default off (resident=True still asks for it explicitly)
    os.environ["EBOS_RESIDENT"] = "0"
    try:
        off = FusedPatchLoop(plan, (24, 32), (24, 32), torch.zeros((2, 4, 4)), 1.0, 0.01, 0.02, halo="auto", lr=0.1, capacity=30)
        np.testing.assert_array_equal(off.run(30).cpu().numpy(), hist["native"])
        assert off.last_run_mode == "pipeline"
    finally:
        del os.environ["EBOS_RESIDENT"]
    with pytest.raises(ValueError):
        loop.run(1)


_VG_OBJECTIVES = {"variance": (1.0, 0.0, 0.0, 0.0), "variance+reg": (2.0, 0.01, 0.05, 0.0), "gm+reg": (0.0, 0.02, 0.03, 1.5)}  # (w_var, w_norm, w_tv, w_gm)
_VG_SHAPE, _VG_PATCH = (96, 128), (24, 32)
_vg_cache = {}


def _vg_events(frac):
    """~20 k events of moving points on the 96 x 128 image; ``frac``: with fractional source coordinates (1/64 px steps)."""
    if frac not in _vg_cache:
        h, w = _VG_SHAPE
        ev = moving_points(h, w, 500, 40, np.array([4.0, -2.5]), seed=6)
        if frac:
            rs = np.random.RandomState(19)
            ev[:, :2] = np.clip(ev[:, :2] + rs.randint(0, 64, (len(ev), 2)) / 64.0, 0, [h - 1, w - 1])
        _vg_cache[frac] = ev
    return _vg_cache[frac]


def _vg_theta0():
    return torch.from_numpy(np.random.RandomState(3).uniform(-2, 2, (2, 4, 4))).float()


def _vg_oracle(objective):
    """(loss, d loss / d theta) of the fp64 oracle's autograd at the start, on the integer-pixel events; once per objective."""
    key = ("oracle", objective)
    if key not in _vg_cache:
        w_var, w_norm, w_tv, w_gm = _VG_OBJECTIVES[objective]
        t64 = _vg_theta0().double().requires_grad_(True)
        dense = O.upsample_patch_flow(t64, _VG_SHAPE, _VG_PATCH, _VG_PATCH)
        iwe = O.iwe_dense(torch.from_numpy(_vg_events(False)), dense, _VG_SHAPE)
        loss = (w_gm * O.gradient_magnitude(iwe) if w_gm else w_var * O.image_variance(iwe)) + w_norm * O.flow_norm(dense)
        loss = loss + w_tv * O.image_gradient_tv(dense, torch.ones(_VG_SHAPE, dtype=torch.float64))
        loss.backward()
        _vg_cache[key] = (loss.item(), t64.grad.numpy().copy())
    return _vg_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("route,objective,masked", [(r, o, False) for r in ("grid", "dense", "frac") for o in _VG_OBJECTIVES]
                         + [("grid", "variance+reg", True)])
def test_patch_gradient_entry_is_the_step_without_the_update(route, objective, masked):
    """``FusedPatchLoop.value_and_grad`` is one ``ebos_cmax_patch_gradient_f32``: the launches of the first Adam step of
    ``ebos_cmax_patch_solve_f32`` ending in the plain adjoint.  On each route (grid sampling on a compact plan, the dense flow field,
    grid sampling on fractional source coordinates) and objective: the loss (1e-6 relative) and d_theta (1e-5 rel-L2) of the first step
    of a twin loop; theta, the Adam state, the step counter and the losses bit for bit what they were -- on a fresh loop and on one that
    has stepped --; on the compact grid route the fp64 oracle's autograd (loss 1e-5, gradient 1e-3 rel-L2); with a ``theta_mask``,
    exactly zero on the masked patches."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = _VG_SHAPE
    w_var, w_norm, w_tv, w_gm = _VG_OBJECTIVES[objective]
    plan = ebos.EventPlan.build(torch.from_numpy(_vg_events(route == "frac")).cuda(), (h, w), "first", True, tile="auto")
    assert plan.compact != (route == "frac")
    theta0 = _vg_theta0()
    mask = None
    if masked:
        mask = torch.ones((4, 4))
        mask[0, 1] = mask[2, 3] = 0.0

    def make():
        return FusedPatchLoop(plan, _VG_PATCH, _VG_PATCH, theta0, w_var, w_norm, w_tv, halo="auto", lr=0.1, capacity=4, w_gradient_magnitude=w_gm,
                              theta_mask=mask, sample_grid=False if route == "dense" else None)

    def state(loop):
        return [t.clone() for t in (loop.theta, loop.exp_avg, loop.exp_avg_sq, loop.step, loop.losses)]

    a, b = make(), make()
    assert a.sample_grid == (route != "dense")
    before = state(a)
    loss, grad = a.value_and_grad(theta0.cuda())
    assert all(torch.equal(x, y) for x, y in zip(before, state(a))) and a.t == 0
    l1 = b.run(1, resident=False).cpu().numpy()
    assert b.last_run_mode == "pipeline"
    d_step = b.d_theta if mask is None else b.d_theta * mask.cuda()
    e_loss, e_grad = abs(float(loss) / float(l1[0]) - 1), float((grad - d_step).norm() / d_step.norm())
    print(f"{route} {objective}: against the first step: loss rel {e_loss:.2e}, d_theta rel-L2 {e_grad:.2e}")
    assert e_loss < 1e-6 and e_grad < 1e-5
    before = state(b)   # ... and on a loop whose Adam state, step counter and losses are not zero
    b.value_and_grad(b.theta.clone())
    assert all(torch.equal(x, y) for x, y in zip(before, state(b))) and b.t == 1
    if route == "grid":
        loss_ref, grad_ref = _vg_oracle(objective)
        if mask is not None:
            grad_ref = grad_ref * mask.numpy()
        e_loss, e_grad = abs(float(loss) - loss_ref) / abs(loss_ref), O.rel_l2(grad.cpu().numpy(), grad_ref)
        print(f"{route} {objective}: against the fp64 oracle: loss rel {e_loss:.2e}, d_theta rel-L2 {e_grad:.2e}")
        assert e_loss <= 1e-5 and e_grad < 1e-3
    if mask is not None:
        assert torch.count_nonzero(grad[:, mask.cuda() == 0]) == 0 and torch.count_nonzero(grad) > 0


@pytest.mark.gpu
def test_solver_recovers_translation_dense_and_2dof():
    import event_based_bos_amd as ebos

    h, w = 96, 128
    v = np.array([6.0, -4.0])
    ev = moving_points(h, w, 600, 40, v, seed=1)
    cfg = load_cfg()["solver"]
    cfg.update(patch={"size": [24, 32], "sliding_window": [24, 32]}, optimizer={"method": "Adam", "n_iter": 80, "parameters": {"lr": 0.5}},
               cost_with_weight={"image_variance": 1.0}, iwe={"method": "bilinear_vote", "blur_sigma": 0})
    cfg["filter"] = {"parameters": {"xmin": 0, "xmax": h, "ymin": 0, "ymax": w}}
    s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    events, period = s.preprocess(ev)
    assert events.shape == ev.shape and abs(period - 0.02) < 1e-3
    flow = s.estimate(events)
    assert flow.shape == (2, h, w) and flow.dtype == np.float64
    assert s.history[-1] < s.history[0] * 1.5  # loss (= -variance) went down (more negative)
    med = np.median(flow.reshape(2, -1), axis=1)
    assert np.all(np.abs(med - v) < 1.0), med
    cfg2 = dict(cfg, motion_model="2d-translation", parameters={"trans_x": {"min": -12, "max": 12}, "trans_y": {"min": -12, "max": 12}},
                optimizer={"method": "grid", "n_iter": 576})
    s2 = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg2)
    flow2 = s2.estimate(ev)
    assert np.allclose(flow2[:, 0, 0], v, atol=0.6), flow2[:, 0, 0]  # dense-flow equivalent of theta = -v
    # a coarse sweep (6 x 6 over +-12: 4 px steps) refined with Adam on the gradient of the 2-DoF kernels
    cfg3 = dict(cfg2, optimizer={"method": "grid", "n_iter": 36, "refine_iters": 40, "parameters": {"lr": 0.2}})
    s3 = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg3)
    flow3 = s3.estimate(ev)
    assert len(s3.history) == 36 + 40 and min(s3.history[36:]) <= min(s3.history[:36])
    assert np.allclose(flow3[:, 0, 0], v, atol=0.6), flow3[:, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [0, 1])
def test_solver_trajectory_matches_cpu_oracle(blur):
    """Same Adam loop, driven once by the HIP pipeline (f32) and once by the CPU oracle (fp64);
    blur = 1 takes the contrast on the 3-tap blurred IWE (the un-fused objective through the blur adjoint)."""
    import event_based_bos_amd as ebos

    h, w, n_iter = 60, 78, 6
    ev = moving_points(h, w, 300, 30, np.array([3.0, 2.0]), seed=2)
    cfg = load_cfg()["solver"]
    cfg.update(patch={"size": [20, 26], "sliding_window": [20, 26]},
               optimizer={"method": "Adam", "n_iter": n_iter, "parameters": {"lr": 0.3}, "graph": True},
               iwe={"method": "bilinear_vote", "blur_sigma": blur})
    s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    s.estimate(ev)
    gh, gw = ebos.solver.patch_grid_shape((h, w), (20, 26), (20, 26))
    theta = torch.zeros((2, gh, gw), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=0.3)
    ref = []
    tev = torch.from_numpy(ev)
    for _ in range(n_iter):
        opt.zero_grad()
        dense = O.upsample_patch_flow(theta, (h, w), (20, 26), (20, 26))
        iwe = O.iwe_dense(tev, dense, (h, w))
        iwe = O.gaussian_blur3_torch(iwe, float(blur)) if blur else iwe
        loss = O.image_variance(iwe) + 0.001 * O.flow_norm(dense)
        loss.backward()
        opt.step()
        ref.append(loss.item())
    np.testing.assert_allclose(s.history, ref, rtol=2e-3)
    np.testing.assert_allclose(s.patch_flow.cpu().numpy(), theta.detach().numpy(), atol=5e-2)
    # both run the fused loop (no autograd graph): blur = 0 as ONE resident launch where the geometry allows it (it does here);
    # blur = 1 natively too -- the blur's image pass between combine and backward (csrc/blur3.h)
    assert s.fused and not s.graphed
    assert s.loop_mode in (("resident",) if blur == 0 else ("resident", "pipeline"))
    cfg_p = dict(cfg, optimizer=dict(cfg["optimizer"], resident=False))
    s_p = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg_p)
    s_p.estimate(ev)
    assert s_p.loop_mode == "pipeline"
    if blur == 0:
        np.testing.assert_array_equal(np.array(s.history), np.array(s_p.history))
    else:  # (the resident loop takes the mean of the blurred image from position-weighted tile sums: agreement to rounding)
        np.testing.assert_allclose(s.history, s_p.history, rtol=2e-5)
    np.testing.assert_allclose(s_p.history, ref, rtol=2e-3)
    # ... and the autograd objective (optimizer.fused: false), graph-replayed and eager: the same trajectory
    cfg_a = dict(cfg, optimizer=dict(cfg["optimizer"], fused=False))
    s_a = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg_a)
    s_a.estimate(ev)
    assert not s_a.fused and s_a.graphed
    np.testing.assert_allclose(s_p.history, s_a.history, rtol=2e-5)
    cfg_e = dict(cfg, optimizer=dict(cfg["optimizer"], fused=False, graph=False))
    s_e = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg_e)
    s_e.estimate(ev)
    assert not s_e.graphed and not s_e.fused
    np.testing.assert_allclose(s_a.history, s_e.history, rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("blur,omit,pad,frac", [(0, False, 0, False), (3, False, 0, False), (1, True, 0, False), (3, False, 2, False),
                                                (3, False, 0, True), (0, True, 1, True)])
def test_translation_adam_loop_is_native_and_matches_cpu_oracle(blur, omit, pad, frac):
    """motion_model 2d-translation + Adam (+ iwe.blur_sigma 3): what the reference's configs/hot_plate1.yaml:47,65,70 selects.  The loop
    runs natively (ebos_cmax_2dof_solve_f32: no host synchronisation per iteration) and follows the fp64 oracle's Adam loop
    (warp_2dof -> bilinear vote -> [gaussian_blur3] -> var, torch.optim.Adam).  frac: fractional source coordinates, as the
    sub-pixel rectification or an earlier warp produces (the reference's loaders hand out integer sensor coordinates) -- the (x, y, dt) plan format."""
    import event_based_bos_amd as ebos

    h, w, n_iter = 60, 78, 12
    ev = moving_points(h, w, 300, 30, np.array([3.0, 2.0]), seed=4)
    if frac:
        ev[:, :2] = np.clip(ev[:, :2] + np.random.RandomState(9).uniform(-0.45, 0.45, (len(ev), 2)), 0, [h - 1, w - 1])
    cfg = load_cfg()["solver"]
    cfg.update(motion_model="2d-translation", cost_with_weight={"image_variance": 1.0}, omit_boundary=omit, outer_padding=pad,
               optimizer={"method": "Adam", "n_iter": n_iter, "parameters": {"lr": 0.2}},
               iwe={"method": "bilinear_vote", "blur_sigma": blur})
    s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    flow = s.estimate(ev)
    assert s.fused and s.loop_mode == "resident"   # (round 6: also with outer_padding -- the windows reach the padding ring)
    theta = torch.zeros(2, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=0.2)
    tev = torch.from_numpy(ev)
    ref = []
    for _ in range(n_iter):
        opt.zero_grad()
        iwe = O.iwe_2dof(tev, theta, (h, w), (pad, pad), "first", True)
        iwe = O.gaussian_blur3_torch(iwe, float(blur)) if blur else iwe
        loss = O.image_variance(iwe, omit)
        loss.backward()
        opt.step()
        ref.append(loss.item())
    np.testing.assert_allclose(s.history, ref, rtol=2e-4)
    np.testing.assert_allclose(-flow[:, 0, 0], theta.detach().numpy(), atol=2e-3)
    # the autograd loop (optimizer.fused: false) is the same objective through the general kernels
    cfg_a = dict(cfg, optimizer=dict(cfg["optimizer"], fused=False))
    s_a = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg_a)
    s_a.estimate(ev)
    assert not s_a.fused
    np.testing.assert_allclose(s.history, s_a.history, rtol=2e-4)


@pytest.mark.gpu
def test_yaml_driven_run_improves_contrast():
    """BASELINE configs[0] plumbing: configs/cmax_hot_plate1.yaml (key names of the reference's hot_plate1.yaml) ->
    solver registry -> preprocess -> estimate, as the reference's driver does (bos_event.py:190-194); the estimated
    flow must sharpen the un-blurred IWE of the 346x260, 100 k-event synthetic window."""
    import json
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_cmax.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["image"] == [260, 346] and rep["iterations"] == 200
    assert rep["loss_last"] < rep["loss_first"]
    assert rep["variance_warped"] > 1.3 * rep["variance_unwarped"], rep


def test_propagate_config_equals_the_reference_on_its_own_yaml():
    """tests/golden/config_hot_plate1.json holds the reference's configs/hot_plate1.yaml as parsed data and what the
    reference's propagate_config (src/utils/config_utils.py:42-88) makes of it: same result, key for key."""
    import copy
    import json

    import event_based_bos_amd as ebos

    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config_hot_plate1.json")))
    cfg = copy.deepcopy(fx["input"])
    assert ebos.utils.propagate_config(cfg) is cfg and cfg == fx["propagated"]
    assert (cfg["data"]["height"], cfg["data"]["width"]) == (720, 1280)                          # :5-6
    assert cfg["solver"]["filter"]["parameters"]["ymin"] == 320 and cfg["data"]["crop_width"] == 640  # :23-26
    # the solver reads it: ROI from the propagated filter parameters, n_iter / method / blur from :46-70, the LIST form of
    # `parameters` (:48-50) with the sampler ranges of optimizer.parameters
    scfg = dict(cfg["solver"], method="contrast_maximization", cost_with_weight={"image_variance": 1.0})
    s = ebos.solver.collections["contrast_maximization"]((720, 1280), (720, 640), solver_config=scfg)
    assert s.roi == (0, 720, 320, 960) and s.motion_model == "2d-translation" and s.warp_direction == "first"
    assert (s.opt_method, s.n_iter, s.blur_sigma, s.pad) == ("Adam", 600, 3.0, 0)
    assert s._param_range("trans_x") == {"min": -30.0, "max": 30.0} and s._param_range("p_x") == {"min": -0.4, "max": 0.4}
    # a config without the optional sections propagates too (the reference would raise KeyError on solver.filter)
    small = {"data": {"height": 260, "width": 346}, "common_params": {"xmin": 0, "xmax": 260, "ymin": 0, "ymax": 346}, "solver": {}}
    ebos.utils.propagate_config(small)
    assert small["solver"]["filter"]["parameters"] == {"xmin": 0, "xmax": 260, "ymin": 0, "ymax": 346}
    assert small["solver"]["crop_height"] == 260 and small["params_openpiv"]["pad_y1"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("size,fractional", [(None, True), ((260, 346), True), ((260, 346), False)])
def test_reference_hot_plate1_config_drives_the_solver(size, fractional):
    """BASELINE configs[0]: the reference's configs/hot_plate1.yaml (fixture: parsed data), consumed key for key by
    tools/run_cmax.py with the driver protocol of bos_event.py:190-194 -- at 720x1280 with the region of interest as the file
    declares it, and at the 346x260 override.  2d-translation + Adam x 600 + blur_sigma 3 come from the file; on sub-pixel event
    coordinates the recovered translation must be the scene's (3, -2) px within 0.75 px and sharpen the IWE.  On integer pixels --
    what the reference's loaders hand out -- the variance has a local optimum at zero flow (an event on a pixel centre is not
    smeared) and Adam, started at zero as src/solver/generative_max_likelihood.py:425-445 starts it, stays there on the synthetic
    window: that run checks the loop (resident, 600 iterations, the same trajectory twice)."""
    import json
    import subprocess
    import sys

    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_cmax.py"), "--config_file",
           os.path.join(ROOT, "tests", "golden", "config_hot_plate1.json")]
    if size:
        cmd += ["--height", str(size[0]), "--width", str(size[1])]
    if fractional:
        cmd += ["--fractional"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["overrides"]["solver.method"] == ["patch_eklt_pyramid2", "contrast_maximization"]
    assert rep["image"] == list(size or (720, 1280)) and rep["crop"] == list(size or (720, 640))
    assert rep["roi"] == ([0, size[0], 0, size[1]] if size else [0, 720, 320, 960])
    assert (rep["motion_model"], rep["optimizer"], rep["iterations"], rep["blur_sigma"]) == ("2d-translation", "Adam", 600, 3.0)
    assert rep["events"] <= rep["events_in"] and (size is not None or rep["events"] < 0.6 * rep["events_in"])  # ROI = half the columns
    assert rep["fused"] and rep["loop_mode"] == "resident"
    if not fractional:
        assert rep["loss_last"] <= rep["loss_first"] + 1e-2 * abs(rep["loss_first"]), rep
        return
    assert rep["loss_last"] < rep["loss_first"] and rep["variance_warped"] > 1.3 * rep["variance_unwarped"], rep
    # estimate() returns the dense flow -theta (src/warp.py:186-187) = the scene's displacement: (3, -2) px plus a bump of up to
    # (6, -3) px in the middle of the frame
    assert 2.5 < rep["flow_mean_in_roi"][0] < 6.5 and -4.0 < rep["flow_mean_in_roi"][1] < -1.5, rep


@pytest.mark.gpu
def test_resident_queries_refuse_a_grid_that_cannot_be_co_resident():
    """720 x 640 (hot_plate1's region of interest) on 32 x 32 tiles is 460 workgroups: more than the device has CUs.  The ``supported``
    queries say so (a refused LAUNCH would raise), and ``run`` takes the four launches."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import Fused2dofLoop, FusedPatchLoop

    h, w, n = 720, 640, 50_000
    rs = np.random.RandomState(0)
    ev = np.stack([rs.randint(0, h, n), rs.randint(0, w, n), np.sort(rs.uniform(0, 0.5, n)), rs.randint(0, 2, n)], 1).astype(np.float64)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile=(32, 32), emit="compact")
    two = Fused2dofLoop(plan, torch.tensor([1.0, -0.5]), 1.0, False, 0, "auto", lr=0.01, capacity=16, blur_sigma=3.0)
    assert not two.resident_supported() and b"co-resident" in ebos.load_library().ebos_last_error()
    two.run(5)
    assert two.last_run_mode == "pipeline"
    gh, gw = ebos.solver.patch_grid_shape((h, w), (24, 32), (24, 32))
    patch = FusedPatchLoop(plan, (24, 32), (24, 32), torch.zeros((2, gh, gw)), 1.0, 0.001, 0.0, halo="auto", lr=0.01, capacity=16)
    assert not patch.resident_supported()
    patch.run(5)
    assert patch.last_run_mode == "pipeline"
    ok = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile=(32, 64), emit="compact")   # 230 workgroups
    assert Fused2dofLoop(ok, torch.tensor([1.0, -0.5]), 1.0, False, 0, "auto", lr=0.01, capacity=16).resident_supported()


@pytest.mark.gpu
def test_window_pipeline_picks_the_tile_for_the_windows_in_flight():
    """At BASELINE configs[0]'s size an iteration of the resident loop is latency, not work: the pipeline takes the resident tile with
    the most workgroups for which the requested windows all fit the device (two windows: 32 x 32 tiles, 99 workgroups each; three
    or four: 32 x 64, 54; eight: 45 x 80, 30 -- given a hardware queue per window, ``_hip.hw_queues()``); a tile named by the solver
    stays; a sensor whose default tile fills the device keeps it.  The flows are those of per-window ``estimate`` on the default
    tile (another tile sums the slabs in another order: 1e-3 px)."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip

    h, w = 260, 346
    cfg = load_cfg()["solver"]
    cfg.update(patch={"size": [20, 26], "sliding_window": [20, 26]}, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.01},
               iwe={"method": "bilinear_vote", "blur_sigma": 0}, optimizer={"method": "Adam", "n_iter": 30, "parameters": {"lr": 0.05}})
    solver = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    assert tuple(solver.plan_tile()) == (32, 32)
    expect = {1: (32, 32), 2: (32, 32), 3: (32, 64), 4: (32, 64), 8: (45, 80) if _hip.hw_queues() >= 10 else (32, 64)}
    if _hip.hw_queues() < 6:  # (shared hardware queues: more than two resident launches would take turns)
        expect = {k: (32, 32) for k in expect}
    for k, tile in expect.items():
        assert ebos.solver.WindowPipeline(solver, n_concurrent=k).tile == tile, (k, tile)
    assert ebos.solver.WindowPipeline(solver, n_concurrent=4, resident=False).tile == (32, 32)
    auto = ebos.solver.WindowPipeline(solver)   # the default: eight in flight where eight resident loops fit side by side, else three
    assert (auto.n_concurrent, auto.tile) == ((8, (45, 80)) if _hip.hw_queues() >= 10 else (4, (32, 32)))
    named = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=dict(cfg, tile=[45, 80]))
    assert ebos.solver.WindowPipeline(named, n_concurrent=3).tile == (45, 80)
    big = ebos.solver.collections["contrast_maximization"]((720, 1280), (720, 1280), solver_config=cfg)
    assert ebos.solver.WindowPipeline(big, n_concurrent=3).tile == (45, 80)
    assert ebos.solver.WindowPipeline(big).n_concurrent == 3
    rs = np.random.RandomState(5)
    n, k_win = 20_000, 4
    store = ebos.data_loader.RawEventStore({"x": rs.randint(0, w, n * k_win).astype(np.int16), "y": rs.randint(0, h, n * k_win).astype(np.int16),
                                            "t": np.sort(rs.randint(0, 8000 * k_win, n * k_win)).astype(np.int32) + 1_000_000,
                                            "p": rs.randint(0, 2, n * k_win).astype(bool)})
    windows = [(i * n, (i + 1) * n) for i in range(k_win)]
    pipe = ebos.solver.WindowPipeline(solver, n_concurrent=3)
    flows = pipe.run(store, windows)
    assert pipe.resident_fallbacks == []
    for wnd, f in zip(windows, flows):
        np.testing.assert_allclose(f, solver.estimate(store.load_event(*wnd)), atol=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("n_concurrent,pyramid", [(1, False), (2, False), (3, True)])
def test_window_pipeline_matches_per_window_estimates(n_concurrent, pyramid):
    """WindowPipeline (raw-column ingest on its own stream, n_concurrent windows solved at once on separate streams by
    ebos_cmax_patch_solve_many_f32) against solver.estimate on the reference-format window, window by window:
    same losses (1e-4 relative over the first 10 iterations, 2e-2 over all) and flows within 0.05 px."""
    import event_based_bos_amd as ebos

    h, w = 96, 128
    rs = np.random.RandomState(11)
    cols, rows, ts, ps, bounds = [], [], [], [], [0]
    for k in range(5):  # five windows of one "recording", each with its own translation
        ev = moving_points(h, w, 400, 30, np.array([3.0 + k, -2.0 + 0.5 * k]), seed=20 + k)
        rows.append(ev[:, 0]); cols.append(ev[:, 1]); ps.append(ev[:, 3])
        ts.append(np.sort(rs.randint(0, 20000, len(ev))) + 1_000_000 + 30000 * k)
        bounds.append(bounds[-1] + len(ev))
    store = ebos.data_loader.RawEventStore({"x": np.concatenate(cols), "y": np.concatenate(rows), "t": np.concatenate(ts),
                                            "p": np.concatenate(ps)})
    windows = [(bounds[k], bounds[k + 1]) for k in range(5)]
    cfg = load_cfg()["solver"]
    patch = {"pyramid": {"coarsest": 32, "finest": 16}} if pyramid else {"size": [24, 32], "sliding_window": [24, 32]}
    cfg.update(patch=patch, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.01},
               iwe={"method": "bilinear_vote", "blur_sigma": 0},
               optimizer={"method": "Adam", "n_iter": 36, "parameters": {"lr": 0.2}})
    solver = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    pipe = ebos.solver.WindowPipeline(solver, n_concurrent=n_concurrent)
    flows = pipe.run(store, windows)
    assert len(flows) == 5 and all(f.shape == (2, h, w) and f.dtype == np.float64 for f in flows)
    # the default runs every window's loop as ONE resident launch; as four launches per iteration (the windows of a group
    # interleaved on streams) the trajectories are the same bit for bit
    assert pipe.resident and pipe.resident_fallbacks == []
    four = ebos.solver.WindowPipeline(solver, n_concurrent=n_concurrent, resident=False)
    flows_four = four.run(store, windows)
    for k in range(5):
        np.testing.assert_array_equal(np.array(pipe.histories[k]), np.array(four.histories[k]))
        np.testing.assert_array_equal(flows[k], flows_four[k])
    # a resident launch that ends early (status != 0: nothing of its window's state changed) -> that window is solved again
    # as four launches; simulated here by a launch that never happens
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    orig, calls = FusedPatchLoop.enqueue_resident, {"n": 0}

    def ends_early(self, n_iter, spin_timeout_s=2.0):
        calls["n"] += 1
        if calls["n"] == 2:
            return torch.full((1,), 2, dtype=torch.int32, device=self.plan.device)
        return orig(self, n_iter, spin_timeout_s)

    FusedPatchLoop.enqueue_resident = ends_early
    try:
        flows_fb = pipe.run(store, windows)
    finally:
        FusedPatchLoop.enqueue_resident = orig
    assert pipe.resident_fallbacks == [1]
    for k in range(5):
        np.testing.assert_array_equal(flows_fb[k], flows[k])
    for k, wnd in enumerate(windows):
        ref = solver.estimate(store.load_event(*wnd))
        assert solver.fused
        dev = np.abs(np.array(pipe.histories[k]) - np.array(solver.history)) / np.abs(np.array(solver.history))
        assert len(pipe.histories[k]) == len(solver.history) and dev[:10].max() < 1e-4 and dev.max() < 2e-2, dev
        assert np.abs(flows[k] - ref).max() < 0.05
    # configurations outside the fused objective family are refused, not silently run differently
    cfg2 = dict(cfg, cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5})
    with pytest.raises(NotImplementedError):
        ebos.solver.WindowPipeline(ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg2)).run(store, windows[:1])
    # iwe.blur_sigma > 0 is part of the family since round 5 (the blur's image pass inside the native loop)
    cfg3 = dict(cfg, iwe={"method": "bilinear_vote", "blur_sigma": 1})
    s3 = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg3)
    f3 = ebos.solver.WindowPipeline(s3, n_concurrent=n_concurrent).run(store, windows[:2])
    for k in range(2):
        ref = s3.estimate(store.load_event(*windows[k]))
        assert s3.fused and np.abs(f3[k] - ref).max() < 0.05


@pytest.mark.gpu
def test_window_pipeline_reads_the_first_groups_verdicts_in_order():
    """the early verdict at the second group is read AFTER the first group's side streams have finished.
    Windows whose events crowd one tile (> 85 k events on a sensor of < 128 tiles) make the resident launches of group 0 really
    end with -104: the later groups must then run as four launches from the start (no second solve), and the results are those
    of a pipeline that never tried the resident kernel."""
    import event_based_bos_amd as ebos

    h, w = 260, 346
    rs = np.random.RandomState(3)
    cols, rows, ts, ps, bounds = [], [], [], [], [0]
    for k in range(4):
        n_c, n_u = 120_000, 15_000   # (> 85 k events on one tile of a small sensor: the launches' window)
        r = np.concatenate([rs.randint(100, 125, n_c), rs.randint(0, h, n_u)])
        c = np.concatenate([rs.randint(200, 222, n_c), rs.randint(0, w, n_u)])
        rows.append(r); cols.append(c); ps.append(rs.randint(0, 2, len(r)))
        ts.append(np.sort(rs.randint(0, 20000, len(r))) + 1_000_000 + 30000 * k)
        bounds.append(bounds[-1] + len(r))
    store = ebos.data_loader.RawEventStore({"x": np.concatenate(cols), "y": np.concatenate(rows), "t": np.concatenate(ts),
                                            "p": np.concatenate(ps)})
    windows = [(bounds[k], bounds[k + 1]) for k in range(4)]
    cfg = load_cfg()["solver"]
    cfg.update(patch={"size": [20, 26], "sliding_window": [20, 26]}, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.01},
               iwe={"method": "bilinear_vote", "blur_sigma": 0}, optimizer={"method": "Adam", "n_iter": 12, "parameters": {"lr": 0.1}})
    solver = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    pipe = ebos.solver.WindowPipeline(solver, n_concurrent=2)
    assert pipe.resident and pipe.n_concurrent == 2
    flows = pipe.run(store, windows)
    assert pipe.resident_fallbacks == [0, 1], pipe.resident_fallbacks          # group 0: -104, solved again as four launches
    assert all(m == ["pipeline"] for m in pipe.window_modes), pipe.window_modes  # groups >= 1: never tried resident
    four = ebos.solver.WindowPipeline(solver, n_concurrent=2, resident=False)
    flows_four = four.run(store, windows)
    # (a crowded tile's upstream window is one sharp peak: bwd_fx_unit gives it the f64 accumulators, whose atomics round in the order
    # they arrive -- the two runs agree to the last bits of a float, not bit for bit)
    for k in range(4):
        np.testing.assert_allclose(np.array(pipe.histories[k]), np.array(four.histories[k]), rtol=1e-5)
        np.testing.assert_allclose(flows[k], flows_four[k], rtol=0, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [{"image_variance": 1.5, "flow_norm": 0.02, "image_gradient": 0.03}, {"gradient_magnitude": 2.0}])
def test_fused_value_and_grad_matches_autograd_and_drives_scipy(terms):
    """FusedPatchLoop.value_and_grad (what the scipy optimisers call for this objective family): same loss (1e-5) and
    patch-flow gradient (rel-L2 1e-4) as the autograd objective at a random non-zero patch flow; and a CG run through
    it lowers the loss."""
    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd import ops

    h, w = 96, 128
    ev = moving_points(h, w, 500, 40, np.array([4.0, -2.5]), seed=8)
    cfg = load_cfg()["solver"]
    cfg.update(patch={"size": [24, 32], "sliding_window": [24, 32]}, cost_with_weight=terms,
               iwe={"method": "bilinear_vote", "blur_sigma": 0}, optimizer={"method": "CG", "n_iter": 25})
    s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto")
    theta = torch.from_numpy(np.random.RandomState(3).uniform(-2, 2, (2, 4, 4))).float().cuda()
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop
    loop = FusedPatchLoop(plan, (24, 32), (24, 32), theta, terms.get("image_variance", 0.0), terms.get("flow_norm", 0.0),
                          terms.get("image_gradient", 0.0), capacity=1, w_gradient_magnitude=terms.get("gradient_magnitude", 0.0))
    loss, grad = loop.value_and_grad(theta)
    t2 = theta.clone().requires_grad_(True)
    ref = s.objective(plan, ops.upsample_patch_flow(t2, (24, 32), (24, 32), (h, w)))
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert float((grad - t2.grad).norm() / t2.grad.norm()) < 1e-4
    s.set_previous_frame_best_estimation(np.full((2, 4, 4), 0.25))
    s.estimate(ev)
    assert s.fused and min(s.history) < s.history[0]


@pytest.mark.gpu
def test_event_thresholding_freezes_sparse_patches():
    """patch.do_event_thresholding / event_thres (src/solver/patch_eklt.py:62-67,118-126): a patch is estimated only when
    MORE than event_thres events fall inside its crop window; the others keep zero flow.  The mask comes from the plan's
    histogram (no per-patch crop_event pass) and equals the reference's loop; the fused loop (grad_mask of the Adam
    kernel), the autograd loop, the scipy path and the window pipeline freeze the same patches."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd import types, utils

    h, w = 96, 128
    ev = moving_points(h, w, 500, 40, np.array([4.0, -2.5]), seed=5)
    ev = ev[~((ev[:, 0] < 48) & (ev[:, 1] >= 64))]          # empty the top-right quadrant ...
    ev = np.concatenate([ev, [[10.0, 100.0, 10.01, 1.0], [30.0, 90.0, 10.012, 0.0]]])  # ... but for two events
    ev = ev[np.argsort(ev[:, 2], kind="stable")]
    patch = slide = (24, 32)
    x0, x1, y0, y1 = types.patch_bounds((h, w), patch, slide)
    counts = np.array([[len(utils.crop_event(ev, x0[a], x1[a], y0[b], y1[b])) for b in range(len(y0))] for a in range(len(x0))])
    thres = 50
    want = counts > thres
    assert 0 < want.sum() < want.size
    flows = {}
    for name, opt in [("fused", {"method": "Adam", "n_iter": 30, "parameters": {"lr": 0.2}, "fused": True}),
                      ("autograd", {"method": "Adam", "n_iter": 30, "parameters": {"lr": 0.2}, "fused": False}),
                      ("scipy", {"method": "L-BFGS-B", "n_iter": 5, "fused": True})]:
        cfg = load_cfg()["solver"]
        cfg.update(patch={"size": list(patch), "sliding_window": list(slide), "do_event_thresholding": True, "event_thres": thres},
                   cost_with_weight={"image_variance": 1.0, "flow_norm": 0.01}, iwe={"method": "bilinear_vote", "blur_sigma": 0},
                   optimizer=opt)
        s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
        if name == "scipy":
            s.set_previous_frame_best_estimation(np.full((2,) + want.shape, 0.25))  # off the kink at zero flow
        s.estimate(ev)
        plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto")
        assert np.array_equal(s.patch_mask(plan, patch, slide).cpu().numpy() > 0, want)
        pf = s.patch_flow.cpu().numpy()
        assert np.all(pf[:, ~want] == 0.0), name                       # frozen patches: exactly zero
        assert np.all(np.abs(pf[:, want]).max(0) > 0.0), name          # the others moved
        flows[name] = pf
    assert np.abs(flows["fused"] - flows["autograd"]).max() < 0.25
    # no thresholding: every patch is estimated
    cfg["patch"]["do_event_thresholding"] = False
    cfg["optimizer"] = {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.2}}
    s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    s.estimate(ev)
    assert np.all(np.abs(s.patch_flow.cpu().numpy()).max(0) > 0.0)
    # the window pipeline applies the same mask
    cfg["patch"]["do_event_thresholding"] = True
    cfg["optimizer"] = {"method": "Adam", "n_iter": 30, "parameters": {"lr": 0.2}}
    solver = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    us = np.round((ev[:, 2] - 10.0) * 1e6).astype(np.int64) + 1_000_000
    store = ebos.data_loader.RawEventStore({"x": ev[:, 1], "y": ev[:, 0], "t": us, "p": ev[:, 3]})
    pipe = ebos.solver.WindowPipeline(solver, n_concurrent=2)
    pipe.run(store, [(0, len(ev))])
    pf = pipe.patch_flows[0].cpu().numpy() if hasattr(pipe.patch_flows[0], "cpu") else np.asarray(pipe.patch_flows[0])
    assert np.all(pf[:, ~want] == 0.0) and np.all(np.abs(pf[:, want]).max(0) > 0.0)


@pytest.mark.gpu
def test_solver_halo_option_selects_the_small_window_configuration():
    """solver.halo: 16 plans the windows on the tile configuration built for that halo (720x1280: 45x80 + 16) and changes
    nothing but the size of the tile-private windows: same losses and flows as halo 32 (displacements beyond a halo are still
    handled, by the spill path -- here none are)."""
    import event_based_bos_amd as ebos

    h, w = 720, 1280
    ev = moving_points(h, w, 3000, 40, np.array([3.0, -2.0]), seed=8)
    out = {}
    for halo in (32, 16):
        cfg = load_cfg()["solver"]
        cfg.update(patch={"size": [48, 64], "sliding_window": [48, 64]}, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.001},
                   iwe={"method": "bilinear_vote", "blur_sigma": 0}, halo=halo,
                   optimizer={"method": "Adam", "n_iter": 25, "parameters": {"lr": 0.2}})
        s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
        assert s.plan_tile() == (45, 80)
        flow = s.estimate(ev)
        assert s.fused
        out[halo] = (np.array(s.history), flow)
    # (values are bit-identical per evaluation; the gradients' fixed-point unit is per tile from max |upstream| over the tile's
    # WINDOW, so two window sizes round differently at the 1e-5 level and 25 Adam steps carry that along)
    np.testing.assert_allclose(out[16][0], out[32][0], rtol=2e-4)
    assert np.abs(out[16][1] - out[32][1]).max() < 5e-3, np.abs(out[16][1] - out[32][1]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,patch,terms", [
    ((96, 128), 20_000, (24, 32), (1.0, 0.01, 0.02)),      # 12 tiles of 32 x 32: the small end (image_gradient on: the apron's cells)
    ((260, 346), 100_000, (20, 20), (1.0, 0.001, 0.0)),    # BASELINE configs[0]'s size: 99 tiles, W % 4 != 0 (scalar image stores)
    ((720, 1280), 400_000, (24, 32), (1.0, 0.001, 0.0)),   # 256 tiles of 45 x 80: one workgroup per CU
    ((720, 640), 300_000, (24, 32), (1.0, 0.001, 0.01)),   # the ROI of configs/hot_plate1.yaml (columns 320:960): 230 tiles of 32 x 64
])
def test_resident_loop_matches_the_four_launch_pipeline(size, n_ev, patch, terms):
    """The loop of src/solver/generative_max_likelihood.py:306-341 as ONE resident launch (ebos_cmax_patch_solve_resident_f32)
    against the four-launch pipeline (ebos_cmax_patch_solve_f32): the first IWE bit for bit (same order of additions), losses to
    1e-6 relative over 300 iterations, patch flows and optimiser state to 1e-5; a resident run can be continued by the pipeline."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = size
    rs = np.random.RandomState(11)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    gh, gw = ebos.solver.patch_grid_shape((h, w), patch, patch)
    theta0 = torch.from_numpy(rs.uniform(-3, 3, (2, gh, gw))).float()
    n_iter = 300

    def make():
        return FusedPatchLoop(plan, patch, patch, theta0, *terms, halo="auto", lr=0.05, capacity=n_iter + 20)

    ref, res = make(), make()
    assert res.resident_supported(), ebos.load_library().ebos_last_error()
    ref.run(1, resident=False)
    res.run(1, resident=True)
    assert res.last_run_mode == "resident" and res.resident_status == 0 and res.resident_iterations == 1
    assert torch.equal(ref.iwe, res.iwe)                                  # the image of the first iteration: same bits
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), rtol=0, atol=1e-6)
    l_ref = ref.run(n_iter - 1, resident=False).cpu().numpy()
    l_res = res.run(n_iter - 1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.t == n_iter and int(res.step.item()) == n_iter
    assert res.resident_iterations == n_iter - 1   # (what the LAST launch completed)
    print("max rel loss deviation", np.abs(l_res / l_ref - 1).max(), "theta", (res.theta - ref.theta).abs().max().item())
    np.testing.assert_allclose(l_res, l_ref, rtol=1e-6)
    np.testing.assert_allclose(ref.losses[:n_iter].cpu().numpy(), res.losses[:n_iter].cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(res.exp_avg.cpu().numpy(), ref.exp_avg.cpu().numpy(), rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(res.d_theta.cpu().numpy(), ref.d_theta.cpu().numpy(), rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(res.variance.cpu().numpy(), ref.variance.cpu().numpy(), rtol=1e-6)
    # continued by the other mode
    a = ref.run(10, resident=True).cpu().numpy()
    b = res.run(10, resident=False).cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,patch,omit,sigma", [
    ((96, 128), 20_000, (24, 32), False, 1.0),      # 12 tiles of 32 x 32
    ((260, 346), 100_000, (20, 20), True, 3.0),     # BASELINE configs[0]'s size, with the boundary ring
    ((720, 1280), 400_000, (24, 32), False, 3.0),   # 256 tiles of 45 x 80
    ((720, 640), 300_000, (24, 32), True, 1.0),     # 230 tiles of 32 x 64
])
def test_resident_loop_with_the_blurred_contrast_matches_the_pipeline(size, n_ev, patch, omit, sigma):
    """iwe.blur_sigma > 0 inside the ONE-launch loop: the resident kernel gathers its upstream window with a 2 px
    apron, blurs it and applies the blur's adjoint in LDS (csrc/blur3.h: the functions of the pipeline's image pass); the mean of
    the blurred image comes from position-weighted tile sums, so the two forms of the loop agree to rounding (1e-6 relative per
    loss over 40 iterations -- Adam's normalised steps amplify a last-bit difference of a near-zero gradient, over hundreds of
    iterations on structure-less events the two trajectories drift apart like any two roundings of the same loop), not bit for bit.
    The raw image that leaves the kernel is the pipeline's bit for bit."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = size
    rs = np.random.RandomState(13)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    gh, gw = ebos.solver.patch_grid_shape((h, w), patch, patch)
    theta0 = torch.from_numpy(rs.uniform(-3, 3, (2, gh, gw))).float()
    n_iter = 40

    def make():
        # (lr: the flows stay below ~8 px over the run -- beyond ~12 px the blurred loop hands over to the pipeline, next test)
        return FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.001, 0.01, omit, halo="auto", lr=0.02, capacity=n_iter + 20, blur_sigma=sigma)

    ref, res = make(), make()
    assert res.resident_supported(), ebos.load_library().ebos_last_error()
    l1_ref = ref.run(1, resident=False).cpu().numpy()
    l1_res = res.run(1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.resident_status == 0 and res.resident_iterations == 1
    assert torch.equal(ref.iwe, res.iwe)
    np.testing.assert_allclose(l1_res, l1_ref, rtol=1e-6)
    np.testing.assert_allclose(res.d_theta.cpu().numpy(), ref.d_theta.cpu().numpy(), rtol=1e-4, atol=1e-8)
    l_ref = ref.run(n_iter - 1, resident=False).cpu().numpy()
    l_res = res.run(n_iter - 1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.t == n_iter and int(res.step.item()) == n_iter
    print("max rel loss deviation", np.abs(l_res / l_ref - 1).max(), "theta", (res.theta - ref.theta).abs().max().item())
    np.testing.assert_allclose(l_res, l_ref, rtol=2e-5)
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), rtol=0, atol=5e-3)
    np.testing.assert_allclose(res.variance.cpu().numpy(), ref.variance.cpu().numpy(), rtol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,patch,omit", [
    ((96, 128), 20_000, (24, 32), False),      # 12 tiles of 32 x 32: every tile touches the image's border
    ((260, 346), 100_000, (20, 20), True),     # BASELINE configs[0]'s size, with the boundary ring; partial last tiles
    ((720, 1280), 400_000, (24, 32), False),   # 256 tiles of 45 x 80
    ((720, 640), 300_000, (24, 32), True),     # 230 tiles of 32 x 64
])
def test_resident_loop_with_the_gradient_magnitude_contrast(size, n_ev, patch, omit):
    """The `gradient_magnitude` contrast (src/costs/gradient_magnitude.py: mean squared Sobel / 8 gradient, replicate padding) inside
    the ONE-launch loop: the resident kernel gathers its upstream window with a 2 px apron, forms the Sobel pairs
    and their adjoint in LDS with the functions of the pipeline's image pass (csrc/sobel3.h).  First iteration against the fp64
    oracle's autograd (loss 1e-5, patch-flow gradient rel-L2 1e-3); against the four-launch pipeline the raw image bit for bit and
    losses / flows to rounding over 60 iterations."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = size
    rs = np.random.RandomState(17)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    gh, gw = ebos.solver.patch_grid_shape((h, w), patch, patch)
    theta0 = torch.from_numpy(rs.uniform(-3, 3, (2, gh, gw))).float()
    n_iter, w_gm, w_norm = 60, 2.0, 0.001

    def make():
        return FusedPatchLoop(plan, patch, patch, theta0, 0.0, w_norm, 0.0, omit, halo="auto", lr=0.02, capacity=n_iter + 20,
                              w_gradient_magnitude=w_gm)

    ref, res = make(), make()
    assert res.resident_supported(), ebos.load_library().ebos_last_error()
    l1_ref = ref.run(1, resident=False).cpu().numpy()
    l1_res = res.run(1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.resident_status == 0 and res.resident_iterations == 1
    assert torch.equal(ref.iwe, res.iwe)
    np.testing.assert_allclose(l1_res, l1_ref, rtol=1e-6)
    print("d_theta: max abs deviation", (res.d_theta - ref.d_theta).abs().max().item(), "of", ref.d_theta.abs().max().item())
    np.testing.assert_allclose(res.d_theta.cpu().numpy(), ref.d_theta.cpu().numpy(), rtol=1e-5, atol=1e-9)
    if n_ev <= 100_000:  # the oracle: fp64 autograd of the same objective at theta0
        t64 = theta0.double().requires_grad_(True)
        dense = O.upsample_patch_flow(t64, (h, w), patch, patch)
        loss = w_gm * O.gradient_magnitude(O.iwe_dense(torch.from_numpy(ev), dense, (h, w)), omit) + w_norm * O.flow_norm(dense)
        loss.backward()
        assert abs(float(l1_res[0]) - loss.item()) <= 1e-5 * abs(loss.item()), (l1_res, loss.item())
        assert O.rel_l2(res.d_theta.cpu().numpy(), t64.grad.numpy()) < 1e-3
    l_ref = ref.run(n_iter - 1, resident=False).cpu().numpy()
    l_res = res.run(n_iter - 1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.t == n_iter and int(res.step.item()) == n_iter
    print("max rel loss deviation", np.abs(l_res / l_ref - 1).max(), "theta", (res.theta - ref.theta).abs().max().item())
    np.testing.assert_allclose(l_res, l_ref, rtol=2e-5)
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), rtol=0, atol=5e-3)
    np.testing.assert_allclose(res.variance.cpu().numpy(), ref.variance.cpu().numpy(), rtol=2e-5)
    # continued by the other mode
    a = ref.run(5, resident=True).cpu().numpy()
    b = res.run(5, resident=False).cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=2e-5)


@pytest.mark.gpu
def test_resident_blurred_loop_hands_over_when_the_windows_outgrow_its_lds_region():
    """The blurred resident loop keeps the raw and the blurred window in the LDS region of the largest upstream window: windows up to
    ~12 px (45 x 80) / ~16 px (32 x 32).  A flow that needs more ends the launch like a spill -- status -102 with the completed
    iterations handed over -- and ``run`` continues with the pipeline: the trajectory is the pipeline's to rounding."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w, n_ev, patch = 96, 128, 20_000, (24, 32)
    rs = np.random.RandomState(12)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    theta0 = torch.full((2, 4, 4), 20.0)   # 20 px: inside the 32 px windows, beyond what the blurred gather keeps in LDS
    ref = FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.01, 0.0, halo="auto", lr=0.05, capacity=16, blur_sigma=1.0)
    res = FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.01, 0.0, halo="auto", lr=0.05, capacity=16, blur_sigma=1.0)
    assert res.resident_supported()
    l_res = res.run(6).cpu().numpy()
    assert res.resident_status == -102 and res.resident_iterations == 0 and res.last_run_mode == "pipeline"
    l_ref = ref.run(6, resident=False).cpu().numpy()
    np.testing.assert_array_equal(l_res, l_ref)
    # ... the gradient-magnitude contrast keeps its raw window and the Sobel pairs the same way: same limit, same hand-over
    ref = FusedPatchLoop(plan, patch, patch, theta0, 0.0, 0.01, 0.0, halo="auto", lr=0.05, capacity=16, w_gradient_magnitude=1.0)
    res = FusedPatchLoop(plan, patch, patch, theta0, 0.0, 0.01, 0.0, halo="auto", lr=0.05, capacity=16, w_gradient_magnitude=1.0)
    assert res.resident_supported()
    l_res = res.run(6).cpu().numpy()
    assert res.resident_status == -102 and res.resident_iterations == 0 and res.last_run_mode == "pipeline"
    np.testing.assert_array_equal(l_res, ref.run(6, resident=False).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,omit,sigma,frac", [((96, 128), 20_000, False, 0.0, False), ((260, 346), 100_000, True, 3.0, False),
                                                       ((720, 1280), 400_000, False, 3.0, False), ((720, 640), 300_000, False, 0.0, False),
                                                       ((260, 346), 100_000, False, 3.0, True), ((720, 1280), 400_000, True, 0.0, True)])
def test_resident_2dof_loop_matches_the_four_launch_loop(size, n_ev, omit, sigma, frac):
    """The 2-DoF Adam loop (configs/hot_plate1.yaml:47: 2d-translation) as ONE resident launch (ebos_cmax_2dof_solve_resident_f32)
    against ebos_cmax_2dof_solve_f32: the first image bit for bit, losses / theta / Adam state to rounding over 150 iterations (the
    tiles' partial pairs are f64 sums of per-lane f64 sums drawn from a dynamic chunk queue: the last bits depend on the draw).
    frac: fractional source coordinates (sub-pixel rectified or pre-warped events) -- both forms read the
    compact layout with the fractions per slot (EventPlan.frac_compact); EBOS_FRAC_GRID=0 puts the launches on the (x, y, dt) arrays."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import Fused2dofLoop

    h, w = size
    rs = np.random.RandomState(14)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    if frac:
        ev[:, :2] = np.clip(ev[:, :2] + rs.randint(0, 64, (n_ev, 2)) / 64.0, 0, [h - 1, w - 1])
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    assert plan.compact == (not frac) and (plan.frac_compact is not None) == frac
    theta0 = torch.tensor([1.5, -2.5])
    n_iter = 150

    def make():
        return Fused2dofLoop(plan, theta0, 1.0, omit, 0, "auto", lr=0.05, capacity=n_iter + 20, blur_sigma=sigma)

    ref, res = make(), make()
    assert res.resident_supported(), ebos.load_library().ebos_last_error()
    l1_ref = ref.run(1, resident=False).cpu().numpy()
    l1_res = res.run(1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.resident_status == 0 and res.resident_iterations == 1
    assert torch.equal(ref.iwe, res.iwe)
    np.testing.assert_allclose(l1_res, l1_ref, rtol=1e-6)
    np.testing.assert_allclose(res.d_theta.cpu().numpy(), ref.d_theta.cpu().numpy(), rtol=1e-4, atol=1e-9)
    if frac:  # the launches on the (x, y, dt) arrays (EBOS_FRAC_GRID=0: x' from the absolute f32 coordinate): the same step to rounding
        os.environ["EBOS_FRAC_GRID"] = "0"
        try:
            xy = make()
            l1_xy = xy.run(1, resident=False).cpu().numpy()
        finally:
            del os.environ["EBOS_FRAC_GRID"]
        np.testing.assert_allclose(l1_xy, l1_ref, rtol=1e-5)
        np.testing.assert_allclose(xy.d_theta.cpu().numpy(), ref.d_theta.cpu().numpy(), rtol=2e-3, atol=1e-7)
    l_ref = ref.run(n_iter - 1, resident=False).cpu().numpy()
    l_res = res.run(n_iter - 1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.t == n_iter and int(res.step.item()) == n_iter
    print("max rel loss deviation", np.abs(l_res / l_ref - 1).max(), "theta", (res.theta - ref.theta).abs().max().item())
    # (frac: the four launches form x' = x + dt theta from the ABSOLUTE coordinate in f32, the resident loop from the fraction --
    # positions differ by ~1e-4 px at x ~ 1000, and 150 normalised Adam steps on structure-less events carry that along)
    np.testing.assert_allclose(l_res, l_ref, rtol=3e-4 if frac else 2e-5)
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), rtol=0, atol=0.2 if frac else 1e-3)
    if not frac:
        np.testing.assert_allclose(res.exp_avg.cpu().numpy(), ref.exp_avg.cpu().numpy(), rtol=2e-2, atol=1e-7)
    np.testing.assert_allclose(res.variance.cpu().numpy(), ref.variance.cpu().numpy(), rtol=3e-4 if frac else 2e-5)
    a = ref.run(10, resident=True).cpu().numpy()      # continued by the other mode
    b = res.run(10, resident=False).cpu().numpy()
    if not frac:
        np.testing.assert_allclose(a, b, rtol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,patch,terms,gm,blur", [
    ((96, 128), 20_000, (24, 32), (1.0, 0.01, 0.02), 0.0, 0.0),       # 12 tiles of 32 x 32, both flow regularisers
    ((260, 346), 100_000, (20, 20), (1.0, 0.001, 0.0), 0.0, 0.0),     # BASELINE configs[0]'s size
    ((720, 1280), 400_000, (24, 32), (0.0, 0.001, 0.0), 1.5, 0.0),    # 256 tiles of 45 x 80, the gradient-magnitude contrast
    ((260, 346), 100_000, (20, 20), (1.0, 0.001, 0.01), 0.0, 3.0),    # iwe.blur_sigma 3 (configs/hot_plate1.yaml:65) on the dense route
    ((96, 128), 20_000, (24, 32), (1.0, 0.0, 0.0), 0.0, 1.0),
])
def test_resident_patch_loop_on_fractional_source_coordinates(size, n_ev, patch, terms, gm, blur):
    """Events rectified with a sub-pixel map (or warped by an earlier stage) have fractional source coordinates.  The natively enqueued
    four-launch loop and the resident launch read the compact layout with the fractions per slot (EventPlan.frac_compact; FRAC
    kernels: general forward loop, f64 backward sweep -- the grid-sampling route), and so does ``value_and_grad``
    (ebos_cmax_patch_gradient_f32: the step's launches, ending in the plain adjoint); ``sample_grid=False`` runs the (x, y, dt)
    arrays through a dense flow field (upsample, general event kernels, adjoint of the upsample).  First iteration against the fp64 oracle's autograd (loss 1e-5, patch-flow gradient rel-L2 1e-3 where the oracle is
    affordable), against the four launches (the same arithmetic: to the last bits of the f64 atomics) and against the dense route
    (which forms x' from the absolute f32 coordinate instead of the fraction: ~1e-4 px apart at x ~ 1000); 60 iterations to
    rounding; a resident run is continued by the four launches."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = size
    rs = np.random.RandomState(19)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    ev[:, :2] = np.clip(ev[:, :2] + rs.randint(0, 64, (n_ev, 2)) / 64.0, 0, [h - 1, w - 1])
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto")
    assert not plan.compact and plan.frac_compact is not None
    gh, gw = ebos.solver.patch_grid_shape((h, w), patch, patch)
    theta0 = torch.from_numpy(rs.uniform(-3, 3, (2, gh, gw))).float()
    n_iter = 60

    def make():
        return FusedPatchLoop(plan, patch, patch, theta0, *terms, halo="auto", lr=0.02, capacity=n_iter + 20, w_gradient_magnitude=gm,
                              blur_sigma=blur)

    ref, res = make(), make()
    assert res.sample_grid and res.resident_supported(), ebos.load_library().ebos_last_error()
    l1_ref = ref.run(1, resident=False).cpu().numpy()
    l1_res = res.run(1, resident=True).cpu().numpy()
    assert ref.last_run_mode == "pipeline" and res.last_run_mode == "resident" and res.resident_status == 0 and res.resident_iterations == 1
    # the dense route on the same window (sample_grid=False: what a tile / sliding window outside ebos_patch_fused_supported gets)
    dense = FusedPatchLoop(plan, patch, patch, theta0, *terms, halo="auto", lr=0.02, capacity=4, w_gradient_magnitude=gm, blur_sigma=blur,
                           sample_grid=False)
    assert not dense.sample_grid
    if not blur:  # ... and the gradient entry on the grid route (what the scipy optimisers drive): the natively enqueued step's numbers
        l_v, g_v = make().value_and_grad(theta0.cuda())
        assert abs(float(l_v) / l1_ref[0] - 1) < 1e-6 and float((g_v - ref.d_theta).norm() / ref.d_theta.norm()) < 1e-5
    l1_dense = dense.run(1, resident=False).cpu().numpy()
    assert abs(l1_dense[0] / l1_ref[0] - 1) < 1e-5 and float((dense.d_theta - ref.d_theta).norm() / ref.d_theta.norm()) < 1e-3
    e_iwe = float((res.iwe - ref.iwe).norm() / ref.iwe.norm())
    e_g = float((res.d_theta - ref.d_theta).norm() / ref.d_theta.norm())
    print(f"first iteration: IWE rel-L2 {e_iwe:.2e}, loss rel {abs(l1_res[0] / l1_ref[0] - 1):.2e}, d_theta rel-L2 {e_g:.2e}")
    assert e_iwe < 1e-5 and abs(l1_res[0] / l1_ref[0] - 1) < 1e-5 and e_g < 1e-3
    if n_ev <= 100_000:  # the oracle: fp64 autograd of the same objective at theta0
        t64 = theta0.double().requires_grad_(True)
        dense = O.upsample_patch_flow(t64, (h, w), patch, patch)
        iwe = O.iwe_dense(torch.from_numpy(ev), dense, (h, w))
        iwe = O.gaussian_blur3_torch(iwe, blur) if blur else iwe
        loss = terms[0] * O.image_variance(iwe) + terms[1] * O.flow_norm(dense)
        if terms[2]:
            loss = loss + terms[2] * O.image_gradient_tv(dense, torch.ones((h, w), dtype=torch.float64))
        loss.backward()
        assert abs(float(l1_res[0]) - loss.item()) <= 1e-5 * abs(loss.item()), (l1_res, loss.item())
        assert O.rel_l2(res.d_theta.cpu().numpy(), t64.grad.numpy()) < 1e-3
    l_ref = ref.run(n_iter - 1, resident=False).cpu().numpy()
    l_res = res.run(n_iter - 1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.t == n_iter and int(res.step.item()) == n_iter
    print("max rel loss deviation", np.abs(l_res / l_ref - 1).max(), "theta", (res.theta - ref.theta).abs().max().item())
    np.testing.assert_allclose(l_res, l_ref, rtol=5e-4)   # (the f64 sweep's LDS atomics round in the order they arrive: run to run the
    # deviation over 60 iterations moved between 4e-5 and 1e-4)
    # (structure-less events: a cell whose gradient is rounding noise takes Adam's +-lr steps in either direction -- a few cells
    # walk apart by up to n_iter x lr while the losses agree to 1e-4; the bulk stays together)
    dev = (res.theta - ref.theta).abs().cpu().numpy()
    assert np.median(dev) < 1e-2 and dev.mean() < 3e-2 and dev.max() <= n_iter * 0.02 + 1e-3, (np.median(dev), dev.mean(), dev.max())
    # continued by the four launches
    b = res.run(5, resident=False).cpu().numpy()
    a = ref.run(5, resident=False).cpu().numpy()
    assert res.last_run_mode == "pipeline"
    np.testing.assert_allclose(a, b, rtol=5e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [True, False])
def test_two_builds_of_a_fractional_window_solve_identically(resident):
    """The binning scatter orders the events of one source pixel as its atomics arrive; the fractional compact layout is put into a
    canonical order (an event takes the slot of its rank by dt, fx, fy: compact_fill_kernel; hot pixels: compact_canon_hot_kernel), so two plans of one window hold the same slots and two
    solves walk the same trajectory bit for bit -- the run sums of the backward sweep see the slot order in their last bits, and
    Adam amplified those into 0.1 px after a few hundred iterations."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w, n_ev, patch = 260, 346, 100_000, (20, 26)
    rs = np.random.RandomState(23)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    ev[:, :2] = np.clip(ev[:, :2] + rs.uniform(0, 1, (n_ev, 2)), 0, [h - 1, w - 1])
    hot = n_ev // 40                            # a hot sensor pixel: 2 500 events, random times, a few fraction pairs (the LDS sort of
    ev[:hot, 0] = 100 + rs.choice([0.25, 0.75], hot)      # compact_canon_hot_kernel; short runs are ranked by the fill itself)
    ev[:hot, 1] = 200 + rs.choice([0.125, 0.5], hot)
    ev[:hot, 2] = rs.uniform(0, 0.5, hot)
    ev = ev[np.argsort(ev[:, 2], kind="stable")]
    gh, gw = ebos.solver.patch_grid_shape((h, w), patch, patch)
    theta0 = torch.from_numpy(rs.uniform(-2, 2, (2, gh, gw))).float()
    runs = []
    for _ in range(3):
        plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto")
        loop = FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.001, 0.0, halo="auto", lr=0.03, capacity=100, blur_sigma=1.0)
        losses = loop.run(80, resident=resident).cpu().numpy().copy()
        assert loop.last_run_mode == ("resident" if resident else "pipeline")
        runs.append([a.cpu().numpy().copy() for a in plan.frac_compact[1:]] + [losses, loop.theta.cpu().numpy().copy()])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a, b)
    # the hot pixel's slots are in the canonical order: ascending (dt, fx, fy)
    th, tw = plan.tile
    f_grp, f_pix, f_dt, f_x, f_y = (a.cpu().numpy() for a in plan.frac_compact)
    t = (100 // th) * (-(-w // tw)) + 200 // tw
    sl = slice(4 * f_grp[t], 4 * f_grp[t + 1])
    sel = (f_pix[sl].astype(np.int64) & 0xffff) == (((100 % th) << 8) | (200 % tw))
    sel &= np.isfinite(f_dt[sl])
    d, x, y = f_dt[sl][sel], f_x[sl][sel], f_y[sl][sel]
    assert len(d) >= hot
    order = np.lexsort((y, x, d))
    np.testing.assert_array_equal(np.stack([d, x, y]), np.stack([d[order], x[order], y[order]]))


@pytest.mark.gpu
def test_resident_loop_ends_on_a_spill_and_the_pipeline_takes_over():
    """A flow whose displacements leave the largest LDS window: the resident launch must END (status -102).  In its FIRST iteration
    it leaves theta and the optimiser state untouched and ``run`` produces the four-launch pipeline's result; when the flow grows
    past the windows in iteration k >= 1 the launch hands over after its k completed iterations (state, losses, step counter of
    k iterations: every workgroup stands in front of the same all-to-all) and the pipeline continues -- the same trajectory
    bit for bit as four launches from the start."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w, n_ev, patch = 96, 128, 20_000, (24, 32)
    rs = np.random.RandomState(12)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    theta0 = torch.full((2, 4, 4), 45.0)   # 45 px > the 32 px window
    ref = FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.01, 0.0, halo="auto", lr=0.05, capacity=16)
    res = FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.01, 0.0, halo="auto", lr=0.05, capacity=16)
    status = res.run_resident(5)
    assert status == -102, status
    assert torch.equal(res.theta, theta0.cuda()) and int(res.step.item()) == 0 and float(res.exp_avg.abs().max()) == 0.0
    l_ref = ref.run(5, resident=False).cpu().numpy()
    l_res = res.run(5).cpu().numpy()                      # default mode: tries resident, falls back
    assert res.last_run_mode == "pipeline" and res.resident_status == -102
    np.testing.assert_array_equal(l_ref, l_res)
    assert torch.equal(ref.theta, res.theta)
    # a flow that GROWS past the windows: theta starts at 30.5 px (inside the 32 px windows) and a large learning rate pushes
    # single cells beyond them after a few steps
    theta1 = torch.full((2, 4, 4), 30.5)
    mk = lambda: FusedPatchLoop(plan, patch, patch, theta1, 1.0, 0.0, 0.0, halo="auto", lr=0.6, capacity=40)
    ref, res = mk(), mk()
    status = res.run_resident(30)
    k = res.resident_iterations
    print("resident launch: status", status, "after", k, "completed iterations")
    assert status == -102 and 1 <= k < 30 and int(res.step.item()) == k
    l_ref = ref.run(k, resident=False).cpu().numpy()   # (no tap has left a window yet: the pipeline is bit-reproducible here)
    np.testing.assert_array_equal(res.losses[:k].cpu().numpy(), l_ref)
    for name in ("theta", "exp_avg", "exp_avg_sq", "d_theta"):
        np.testing.assert_array_equal(getattr(ref, name).cpu().numpy(), getattr(res, name).cpu().numpy(), err_msg=name)
    # ... and ``run`` continues with the four launches (whose spill path adds with global float atomics: agreement to rounding)
    ref, res = mk(), mk()
    l_ref = ref.run(30, resident=False).cpu().numpy()
    l_res = res.run(30).cpu().numpy()
    assert res.resident_status == -102 and res.resident_iterations == k and res.last_run_mode == "resident+pipeline"
    assert res.t == 30 and int(res.step.item()) == 30
    np.testing.assert_allclose(l_res, l_ref, rtol=1e-4)
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), atol=1e-2)


def test_crowded_window_rule_follows_the_measured_cross_overs():
    """`crowded_for_resident` (the host's copy of the resident kernels' own verdict) on the windows of profiles/r06t_crowding_rule.json:
    every window goes where it was measured faster.  (1280 x 720 on 45 x 80 tiles: 256 tiles; 346 x 260 on 32 x 32: 99.)"""
    import types

    from event_based_bos_amd.solver.fused_loop import crowded_for_resident

    def plan(size, tile, n, ratio):
        n_tiles = -(-size[0] // tile[0]) * -(-size[1] // tile[1])
        p = types.SimpleNamespace(image_size=size, tile=tile, n=n)
        p.__dict__["_fullest_tile"] = int(ratio * n / n_tiles)
        return p

    big, small = ((720, 1280), (45, 80)), ((260, 346), (32, 32))
    # (events, fullest / average tile, faster on the four launches?)
    for n, ratio, launches in [(1_000_000, 10.6, False), (1_000_000, 21.4, True), (2_000_000, 8.5, False), (2_000_000, 10.7, True),
                               (2_000_000, 21.4, True), (5_000_000, 4.1, False), (5_000_000, 6.2, True), (10_000_000, 2.0, False),
                               (10_000_000, 6.2, True)]:
        assert crowded_for_resident(plan(*big, n, ratio)) == launches, (n, ratio)
    for n, ratio, launches in [(100_000, 41.0, False), (300_000, 23.3, False), (300_000, 40.9, True), (1_000_000, 5.6, False),
                               (1_000_000, 11.4, True)]:
        assert crowded_for_resident(plan(*small, n, ratio)) == launches, (n, ratio)
    unknown = plan(*big, 2_000_000, 30.0)
    unknown.__dict__["_fullest_tile"] = None   # a plan built without its read-back: the kernel decides in its first iteration
    assert not crowded_for_resident(unknown)


@pytest.mark.gpu
def test_resident_loop_leaves_crowded_windows_to_the_pipeline():
    """The resident kernel runs ONE workgroup per tile; the four-launch pipeline splits crowded tiles over several work items.  A
    window whose fullest tile holds more than 60 k + 0.8 % of the window's events (sensors of >= 128 tiles; smaller ones: more than
    12 x the average tile's events and >= 32 k of them) ends the resident launch in its first iteration (status -104, nothing changed)
    and the pipeline runs -- 120 against 61 us per iteration measured with 2 M events in a Gaussian blob of sigma 100 px.  The verdict is the kernel's own (every workgroup sees every tile's count in the records of
    the first all-to-all): it also covers plans built without a host read-back."""
    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w, n = 720, 1280, 600_000
    rs = np.random.RandomState(9)
    r = np.clip(np.rint(rs.normal(h / 2, 20, n)), 0, h - 1)
    c = np.clip(np.rint(rs.normal(w / 2, 36, n)), 0, w - 1)
    ev = np.stack([r, c, np.sort(rs.uniform(0, 0.5, n)), rs.randint(0, 2, n)], 1).astype(np.float64)
    # (a plan built WITH the host read-back knows its fullest tile: the host applies the same rule and never launches)
    known = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    gh, gw = ebos.solver.patch_grid_shape((h, w), (24, 32), (24, 32))
    early = FusedPatchLoop(known, (24, 32), (24, 32), torch.zeros((2, gh, gw)), 1.0, 0.001, 0.0, halo="auto", lr=0.05, capacity=24)
    assert not early.resident_supported()
    early.run(2)
    assert early.last_run_mode == "pipeline" and early.resident_status == 0
    # ... a plan built without it (build_raw(..., deferred=True): what WindowPipeline builds) does not -- here: the same build, told to forget
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    plan.__dict__["_fullest_tile"] = None
    ref = FusedPatchLoop(plan, (24, 32), (24, 32), torch.zeros((2, gh, gw)), 1.0, 0.001, 0.0, halo="auto", lr=0.05, capacity=24)
    res = FusedPatchLoop(plan, (24, 32), (24, 32), torch.zeros((2, gh, gw)), 1.0, 0.001, 0.0, halo="auto", lr=0.05, capacity=24)
    assert res.resident_supported()
    l_ref = ref.run(8, resident=False).cpu().numpy()
    l_res = res.run(8).cpu().numpy()
    assert res.resident_status == -104 and res.last_run_mode == "pipeline"
    np.testing.assert_array_equal(l_res, l_ref)
    res.run(8)                                   # ... and the window is not tried again
    assert res.last_run_mode == "pipeline" and res.t == 16
    os.environ["EBOS_RESIDENT_MAX_IMBALANCE"] = "0"   # the caller's override: never refuse
    try:
        forced = FusedPatchLoop(plan, (24, 32), (24, 32), torch.zeros((2, gh, gw)), 1.0, 0.001, 0.0, halo="auto", lr=0.05, capacity=24)
        l_forced = forced.run(8).cpu().numpy()
        assert forced.last_run_mode == "resident" and forced.resident_status == 0
        np.testing.assert_allclose(l_forced, l_ref, rtol=1e-5)   # (adaptive work items sum a crowded tile's slabs in another order)
    finally:
        del os.environ["EBOS_RESIDENT_MAX_IMBALANCE"]


@pytest.mark.gpu
def test_resident_loop_spins_are_bounded():
    """Every wait of the resident kernel is capped.  Staged here: a one-wave kernel spinning on another stream keeps ONE compute
    unit from taking its workgroup of a 256-tile grid (a resident workgroup needs the whole register file of its CU), so the other
    255 wait for a record that does not come: the launch must END with status -101 after the cap (never hang), leave the patch flow,
    the optimiser state and the step counter untouched, and the four-launch pipeline must then run from that state -- the same
    losses as a loop that never tried."""
    import time

    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = 720, 1280
    rs = np.random.RandomState(5)
    ev = np.stack([rs.randint(0, h, 200_000), rs.randint(0, w, 200_000), np.sort(rs.uniform(0, 0.5, 200_000)), rs.randint(0, 2, 200_000)], 1)
    plan = ebos.EventPlan.build(torch.from_numpy(ev.astype(np.float64)).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    assert plan.tile == (45, 80)
    gh, gw = ebos.solver.patch_grid_shape((h, w), (24, 32), (24, 32))
    theta0 = torch.from_numpy(rs.uniform(-1, 1, (2, gh, gw))).float()
    ref = FusedPatchLoop(plan, (24, 32), (24, 32), theta0, 1.0, 0.001, 0.0, halo="auto", lr=0.1, capacity=16)
    res = FusedPatchLoop(plan, (24, 32), (24, 32), theta0, 1.0, 0.001, 0.0, halo="auto", lr=0.1, capacity=16)
    assert res.resident_supported()
    res.run(1)                      # (warm: module load, LDS attribute, mailbox)
    assert res.last_run_mode == "resident"
    res = FusedPatchLoop(plan, (24, 32), (24, 32), theta0, 1.0, 0.001, 0.0, halo="auto", lr=0.1, capacity=16)
    torch.cuda.synchronize()
    status = 0
    for attempt in range(6):  # (two streams may share a hardware queue: the launch then simply runs after the spinning kernel)
        blocker = torch.cuda.Stream()
        t0 = time.perf_counter()
        with torch.cuda.stream(blocker):
            torch.cuda._sleep(int(4e8))   # one wave, a few hundred ms
        status = res.run_resident(8, spin_timeout_s=0.02)
        waited = time.perf_counter() - t0
        torch.cuda.synchronize()
        print(f"resident launch beside a spinning wave: status {status} after {waited * 1e3:.1f} ms (blocker done after {(time.perf_counter() - t0) * 1e3:.1f} ms)")
        assert waited < 5.0
        if status != 0:
            break
        res = FusedPatchLoop(plan, (24, 32), (24, 32), theta0, 1.0, 0.001, 0.0, halo="auto", lr=0.1, capacity=16)
    if status == 0:
        pytest.skip("the spinning kernel never ran beside the resident launch (shared hardware queue): no timeout to observe")
    assert status == -101, status
    assert res.t == 0 and int(res.step.item()) == 0
    np.testing.assert_array_equal(res.theta.cpu().numpy(), theta0.numpy())
    assert float(res.exp_avg.abs().max()) == 0.0 and float(res.exp_avg_sq.abs().max()) == 0.0
    l_ref = ref.run(8, resident=False).cpu().numpy()
    l_res = res.run(8).cpu().numpy()    # the default mode, now unobstructed: resident
    assert res.last_run_mode == "resident" and res.resident_status == 0
    np.testing.assert_array_equal(l_res, l_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,patch,amp", [((96, 128), 20_000, (24, 32), 20.0), ((720, 1280), 400_000, (24, 32), 24.0)])
def test_resident_loop_with_windows_that_reach_two_tiles_far(size, n_ev, patch, amp):
    """Flows whose LDS windows are larger than half a tile: a halo pixel may then receive events of a tile TWO away, which the
    3 x 3 slabs around a workgroup do not hold -- the resident kernel must notice (every record of the all-to-all carries its
    window), publish the image tiles and stage the halo from them; same losses and flows as the four-launch pipeline, bit for bit."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = size
    rs = np.random.RandomState(13)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    gh, gw = ebos.solver.patch_grid_shape((h, w), patch, patch)
    theta0 = torch.from_numpy(rs.uniform(-amp, amp, (2, gh, gw))).float()
    ref = FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.001, 0.0, halo="auto", lr=0.01, capacity=64)
    res = FusedPatchLoop(plan, patch, patch, theta0, 1.0, 0.001, 0.0, halo="auto", lr=0.01, capacity=64)
    l_ref = ref.run(40, resident=False).cpu().numpy()
    l_res = res.run(40, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.resident_status == 0
    np.testing.assert_array_equal(l_res, l_ref)
    assert torch.equal(ref.theta, res.theta) and torch.equal(ref.iwe, res.iwe)


@pytest.mark.gpu
def test_pyramid_runs_resident_at_every_scale_at_1280x720():
    """The reference's pyramid halves the patch 64 -> 8 and gives the finest scale the most iterations
    (src/solver/patch_eklt_pyramid2.py:55-83,260).  At 1280 x 720 (tiles of 45 x 80) the finest scale's cell block has 234
    elements per tile: every scale runs as ONE resident launch, and the trajectory is the four-launch pipeline's
    bit for bit."""
    import event_based_bos_amd as ebos

    h, w = 720, 1280
    ev = moving_points(h, w, 50_000, 40, np.array([3.0, -2.0]), seed=5)   # 2 M events
    cfg = load_cfg()["solver"]
    cfg.update(patch={"pyramid": {"coarsest": 64, "finest": 8}}, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.001},
               iwe={"method": "bilinear_vote", "blur_sigma": 0}, optimizer={"method": "Adam", "n_iter": 40, "parameters": {"lr": 0.05}})
    s = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    assert [p[0] for p in s.pyramid_scales()] == [(64, 64), (32, 32), (16, 16), (8, 8)]
    flow = s.estimate(ev)
    assert s.fused and s.loop_modes == ["resident"] * 4, s.loop_modes
    cfg_p = dict(cfg, optimizer=dict(cfg["optimizer"], resident=False))
    s_p = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg_p)
    flow_p = s_p.estimate(ev)
    assert s_p.loop_modes == ["pipeline"] * 4
    np.testing.assert_array_equal(np.array(s.history), np.array(s_p.history))
    np.testing.assert_array_equal(flow, flow_p)
    # the same recording with fractional source coordinates (sub-pixel rectified) with the YAMLs' blur: every scale resident too
    # (FRAC kernels), against the launches of the dense route to rounding
    rs = np.random.RandomState(2)
    evf = ev.copy()
    evf[:, :2] = np.clip(evf[:, :2] + rs.randint(0, 64, (len(ev), 2)) / 64.0, 0, [h - 1, w - 1])
    cfg_f = dict(cfg, iwe={"method": "bilinear_vote", "blur_sigma": 1})
    s_f = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg_f)
    s_f.estimate(evf)
    assert s_f.fused and s_f.loop_modes == ["resident"] * 4, s_f.loop_modes
    s_fp = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=dict(cfg_f, optimizer=dict(cfg["optimizer"], resident=False)))
    s_fp.estimate(evf)
    assert s_fp.fused and s_fp.loop_modes == ["pipeline"] * 4
    np.testing.assert_allclose(np.array(s_f.history), np.array(s_fp.history), rtol=2e-3)


@pytest.mark.gpu
def test_fuzz_resident_loops_against_the_launches_and_the_oracle():
    """Seeded fuzz of the ONE-launch loops over what interacts inside the resident kernels: image size (tiles cut by the border, one
    to ~60 tiles, the three resident tile shapes), patch size and sliding window (overlapping patches, cells shared by several
    tiles), event clustering (blobs, borders), integer and fractional source coordinates, the contrast (variance, blurred variance,
    gradient magnitude), both flow regularisers, the boundary ring, the motion model (patch grid / 2-DoF).  Three iterations as one
    resident launch against the same iterations as launches: the first loss to 1e-5, the flows to a small multiple of lr; and the first
    iteration against the fp64 oracle's autograd: loss 1e-5, gradient rel-L2 1e-2 (and 1e-4 against the launches' gradient)."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import Fused2dofLoop, FusedPatchLoop

    lib = ebos.load_library()
    rs = np.random.RandomState(int(os.environ.get("EBOS_FUZZ_SEED", 515)))
    done = {"patch": 0, "2dof": 0, "frac": 0, "gm": 0, "blur": 0}
    for case in range(48):
        h, w = int(rs.randint(40, 300)), int(rs.randint(48, 400))
        n = int(rs.choice([300, 5000, 40000]))
        kind = rs.randint(3)
        if kind == 0:
            r, c = rs.randint(0, h, n), rs.randint(0, w, n)
        elif kind == 1:   # a blob (moderately crowded tiles: the launch must not refuse)
            r, c = np.clip(np.rint(rs.normal(h / 2, h / 5, n)), 0, h - 1), np.clip(np.rint(rs.normal(w / 3, w / 5, n)), 0, w - 1)
        else:             # the image's borders
            r, c = rs.choice([0, 1, h - 2, h - 1], n), rs.randint(0, w, n)
        ev = np.stack([r, c, np.sort(rs.uniform(2.0, 2.4, n)), rs.randint(0, 2, n)], 1).astype(np.float64)
        frac = bool(rs.randint(3) == 0)
        if frac:
            ev[:, :2] = np.clip(ev[:, :2] + rs.randint(0, 64, (n, 2)) / 64.0, 0, [h - 1, w - 1])
        model = "2dof" if rs.randint(3) == 0 else "patch"
        contrast = ["var", "blur", "gm"][rs.randint(3)] if model == "patch" else ["var", "blur"][rs.randint(2)]
        sigma = float(rs.choice([1.0, 3.0])) if contrast == "blur" else 0.0
        omit = bool(rs.randint(2))
        amp = float(rs.choice([0.5, 3.0, 6.0]))
        plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto")
        tag = f"case {case}: {h}x{w} tile {plan.tile} n {n} kind {kind} frac {frac} {model} {contrast} sigma {sigma} omit {omit} amp {amp}"
        if model == "patch":
            patch = (int(rs.randint(8, 40)), int(rs.randint(8, 48)))
            slide = (int(rs.randint(max(4, patch[0] // 2), patch[0] + 1)), int(rs.randint(max(4, patch[1] // 2), patch[1] + 1)))
            if patch[0] > h or patch[1] > w or not lib.ebos_patch_fused_supported(plan.tile[0], plan.tile[1], 32, slide[0], slide[1]):
                continue
            gh, gw = ebos.solver.patch_grid_shape((h, w), patch, slide)
            theta0 = rs.uniform(-amp, amp, (2, gh, gw))
            w_norm, w_tv = [(0.0, 0.0), (0.02, 0.0), (0.01, 0.02)][rs.randint(3)]
            w_var, w_gm = (0.0, 1.5) if contrast == "gm" else (2.0, 0.0)
            tag += f" patch {patch} slide {slide} reg {(w_norm, w_tv)}"

            def make():
                return FusedPatchLoop(plan, patch, slide, torch.from_numpy(theta0).float(), w_var, w_norm, w_tv, omit, halo="auto", lr=0.01,
                                      capacity=8, w_gradient_magnitude=w_gm, blur_sigma=sigma)
        else:
            theta0 = rs.uniform(-amp, amp, 2)

            def make():
                return Fused2dofLoop(plan, torch.from_numpy(theta0).float(), 2.0, omit, 0, "auto", lr=0.01, capacity=8, blur_sigma=sigma)
        ref, res = make(), make()
        if not res.resident_supported():
            continue
        l_res = res.run(3, resident=True).cpu().numpy()
        if res.last_run_mode != "resident":   # (a crowded window: refused in its first iteration -- the launches ran)
            assert res.resident_status in (-102, -104), (tag, res.resident_status)
            continue
        l_ref = ref.run(3, resident=False).cpu().numpy()
        assert abs(l_res[0] / l_ref[0] - 1) < 1e-5, (tag, l_res, l_ref)
        np.testing.assert_allclose(l_res, l_ref, rtol=2e-3, err_msg=tag)
        assert (res.theta - ref.theta).abs().max().item() <= 2 * 3 * 0.01 + 1e-6, tag   # (a near-zero gradient may step either way)
        # the oracle: the first iteration's loss and gradient
        tev = torch.from_numpy(ev)
        if model == "patch":
            t64 = torch.from_numpy(theta0).float().double().requires_grad_(True)
            dense = O.upsample_patch_flow(t64, (h, w), patch, slide)
            iwe = O.iwe_dense(tev, dense, (h, w))
        else:
            t64 = torch.from_numpy(theta0).float().double().requires_grad_(True)
            iwe = O.iwe_2dof(tev, t64, (h, w))
        iwe = O.gaussian_blur3_torch(iwe, sigma) if sigma else iwe
        if contrast == "gm":
            loss = w_gm * O.gradient_magnitude(iwe, omit)
        else:
            loss = 2.0 * O.image_variance(iwe, omit)
        if model == "patch" and (w_norm or w_tv):
            loss = loss + w_norm * O.flow_norm(dense) + w_tv * O.image_gradient_tv(dense, torch.ones((h, w), dtype=torch.float64))
        loss.backward()
        res1 = make()
        l1 = res1.run(1, resident=True).cpu().numpy()
        assert res1.last_run_mode == "resident", tag
        assert abs(float(l1[0]) - loss.item()) <= 1e-5 * abs(loss.item()) + 1e-9, (tag, l1, loss.item())
        want = t64.grad.numpy()
        if n >= 5000 and np.linalg.norm(want) > 0:
            # (the bar of the flow gradient is 1e-3 on BASELINE's configurations; a fuzzed case may sit next to a stationary point,
            # where the gradient is the small difference of large per-event terms and f32's share of it grows: what is pinned tightly
            # here is that the resident launch computes what the launches compute -- their common deviation stays below 1e-2)
            got = res1.d_theta.cpu().numpy().reshape(want.shape)
            ref1 = make()
            ref1.run(1, resident=False)
            assert O.rel_l2(got, ref1.d_theta.cpu().numpy().reshape(want.shape)) < 1e-4, tag
            assert O.rel_l2(got, want) < 1e-2, (tag, O.rel_l2(got, want))
        done[model] += 1
        done["frac"] += frac
        done["gm"] += contrast == "gm"
        done["blur"] += contrast == "blur"
    print("cases run:", done)
    assert done["patch"] >= 10 and done["2dof"] >= 5 and done["frac"] >= 5 and done["gm"] >= 3 and done["blur"] >= 5, done


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [0.0, 3.0])
def test_window_pipeline_drives_the_2dof_adam_loop(blur):
    """The reference's shipped YAML selects the 2-DoF model with Adam (configs/hot_plate1.yaml:47,70): the pipeline runs that loop too,
    one resident launch per window, several windows side by side -- the theta and losses of per-window ``estimate`` (the pipeline
    picks its own tile and reads the raw sensor columns: sums in another order, 1e-4 relative)."""
    import event_based_bos_amd as ebos

    h, w = 260, 346
    rs = np.random.RandomState(9)
    n, k_win = 30_000, 5
    store = ebos.data_loader.RawEventStore({"x": rs.randint(0, w, n * k_win).astype(np.int16), "y": rs.randint(0, h, n * k_win).astype(np.int16),
                                            "t": np.sort(rs.randint(0, 8000 * k_win, n * k_win)).astype(np.int32) + 1_000_000,
                                            "p": rs.randint(0, 2, n * k_win).astype(bool)})
    windows = [(i * n, (i + 1) * n) for i in range(k_win)]
    cfg = load_cfg()["solver"]
    cfg.update(motion_model="2d-translation", parameters=["trans_x", "trans_y"], cost_with_weight={"image_variance": 1.0},
               iwe={"method": "bilinear_vote", "blur_sigma": blur}, optimizer={"method": "Adam", "n_iter": 50, "parameters": {"lr": 0.05}})
    solver = ebos.solver.collections["contrast_maximization"]((h, w), (h, w), solver_config=cfg)
    pipe = ebos.solver.WindowPipeline(solver, n_concurrent=3)
    flows = pipe.run(store, windows)
    assert pipe.resident_fallbacks == [] and all(m == ["resident"] for m in pipe.window_modes)
    four = ebos.solver.WindowPipeline(solver, n_concurrent=3, resident=False).run(store, windows)
    for k, wnd in enumerate(windows):
        ref = solver.estimate(store.load_event(*wnd))
        assert flows[k].shape == (2, h, w) and solver.loop_mode == "resident"
        np.testing.assert_allclose(np.array(pipe.histories[k]), np.array(solver.history), rtol=1e-4)
        np.testing.assert_allclose(flows[k], ref, atol=2e-3)
        np.testing.assert_allclose(four[k], ref, atol=2e-3)


@pytest.mark.gpu
def test_random_sampler_sweep_matches_the_cpu_restatement():
    """``optimizer.method: optuna`` + ``sampler: random`` (src/solver/generative_max_likelihood.py:220-221, configs/hot_plate1.yaml:69):
    n_iter uniform draws inside parameters.{min, max}, seedable, evaluated as one batched 2-DoF sweep.  The best of 512 draws on a
    100 k-event window is the argmax of the oracle's fp64 contrast over the SAME draws, and every contrast agrees to fp32 rounding."""
    import event_based_bos_amd as ebos
    from oracle import ebos_oracle as O

    h, w = 260, 346
    v = np.array([5.0, -3.0])
    ev = moving_points(h, w, 2500, 40, v, seed=3)
    assert len(ev) > 95_000
    cfg = load_cfg()["solver"]
    cfg.update(motion_model="2d-translation", parameters={"trans_x": {"min": -12, "max": 12}, "trans_y": {"min": -12, "max": 12}},
               optimizer={"method": "optuna", "sampler": "random", "n_iter": 512, "seed": 11},
               cost_with_weight={"image_variance": 1.0}, iwe={"method": "bilinear_vote", "blur_sigma": 0})
    s = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg)
    flow = s.estimate(ev)
    draws = np.random.RandomState(11).uniform([-12, -12], [12, 12], (512, 2)).astype(np.float32)
    assert np.array_equal(s.sweep_grid.cpu().numpy(), draws) and len(s.history) == 512
    evt = torch.from_numpy(ev)
    # the solver maximises contrast(theta) with theta the 2-DoF warp parameter (x' = x + dt theta); normalised time as the solvers use
    cpu = np.array([float(O.image_variance(O.iwe_2dof(evt, torch.from_numpy(d.astype(np.float64)), (h, w), normalize_t=True),
                                           omit_boundary=s.omit_boundary, direction="maximize")) for d in draws])
    gpu = s.sweep_contrast.double().cpu().numpy()
    np.testing.assert_allclose(gpu, cpu, rtol=2e-5)
    best = int(np.argmax(cpu))
    assert int(np.argmax(gpu)) == best
    np.testing.assert_allclose(flow[:, 0, 0], -draws[best], atol=1e-6)   # dense flow equivalent of theta (src/warp.py:186-187)
    assert np.all(np.abs(flow[:, 0, 0] - v) < 1.5)                       # ... and 512 draws over +-12 px land near the scene's motion
    # same seed, same draws; method "random" is the sampler's name as the method; no seed = fresh draws (optuna's default)
    s2 = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=dict(cfg, optimizer={"method": "random", "n_iter": 512, "seed": 11}))
    assert np.array_equal(s2.estimate(ev), flow)
    cfg_ref = dict(cfg, optimizer={"method": "random", "n_iter": 64, "seed": 11, "refine_iters": 30, "parameters": {"lr": 0.1}})
    s3 = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg_ref)
    s3.estimate(ev)
    assert len(s3.history) == 64 + 30 and min(s3.history[64:]) <= min(s3.history[:64]) + 1e-6
    with pytest.raises(NotImplementedError):
        ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=dict(cfg, optimizer={"method": "optuna", "sampler": "cmaes"})).estimate(ev)


@pytest.mark.gpu
def test_tpe_sampler_concentrates_its_trials_on_the_optimum():
    """``sampler: TPE`` (:216-219), batched: max(10, n_iter // 10) uniform start-up trials, then Parzen-estimator rounds.  Parity with
    optuna's own stream is unpinned (optuna is not installed here); what is checked: the trial count, the start-up draws, reproducibility
    under a seed, and that the later trials sit closer to the optimum than the uniform start-up ones and find a better contrast."""
    import event_based_bos_amd as ebos

    h, w = 96, 128
    v = np.array([6.0, -4.0])
    ev = moving_points(h, w, 600, 40, v, seed=1)
    cfg = load_cfg()["solver"]
    cfg.update(motion_model="2d-translation", parameters={"trans_x": {"min": -12, "max": 12}, "trans_y": {"min": -12, "max": 12}},
               optimizer={"method": "optuna", "sampler": "TPE", "n_iter": 300, "seed": 5},
               cost_with_weight={"image_variance": 1.0}, iwe={"method": "bilinear_vote", "blur_sigma": 0})
    s = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg)
    flow = s.estimate(ev)
    grid = s.sweep_grid.cpu().numpy()
    assert grid.shape == (300, 2) and len(s.history) == 300
    assert np.array_equal(grid[:30], np.random.RandomState(5).uniform([-12, -12], [12, 12], (30, 2)).astype(np.float32))
    d = np.linalg.norm(grid + v, axis=1)      # theta = -flow: distance of each trial from the scene's motion
    assert np.median(d[150:]) < 0.5 * np.median(d[:30])
    assert min(s.history[30:]) < min(s.history[:30])
    assert np.all(np.abs(flow[:, 0, 0] - v) < 1.0), flow[:, 0, 0]
    s2 = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg)
    assert np.array_equal(s2.estimate(ev), flow)


@pytest.mark.gpu
def test_integer_pixel_2dof_loop_recovers_the_translation_from_a_warm_start():
    """Events on integer sensor pixels (what the reference's loaders hand out): started at zero the variance sits in a local optimum
    (an event on a pixel centre is not smeared), which the hot_plate1 run above only times.  From a warm start -- the driver's
    ``set_previous_frame_best_estimation`` (src/solver/base.py:355-361) -- or from a coarse grid, the resident integer-coordinate loop
    must walk to the scene's translation, along the four launches' trajectory."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import Fused2dofLoop

    h, w = 260, 346
    v = np.array([3.0, -2.0])
    ev = moving_points(h, w, 2500, 40, v, seed=2)
    cfg = load_cfg()["solver"]
    cfg.update(motion_model="2d-translation", optimizer={"method": "Adam", "n_iter": 300, "parameters": {"lr": 0.02}},
               cost_with_weight={"image_variance": 1.0}, iwe={"method": "bilinear_vote", "blur_sigma": 3})
    s = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg)
    s.previous_best = np.array([-1.8, 1.1])   # theta = -flow: a previous window's estimate, 1.5 px off
    flow = s.estimate(ev)
    assert s.fused and s.loop_mode == "resident"
    assert np.all(np.abs(flow[:, 0, 0] - v) < 0.75), flow[:, 0, 0]
    assert s.history[-1] < s.history[0] and np.abs(flow).max() < 30.0
    # the same loop as four launches per iteration: the same trajectory
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile=s.plan_tile(), emit="compact")
    runs = []
    for resident in (True, False):
        loop = Fused2dofLoop(plan, torch.tensor([-1.8, 1.1]), 1.0, s.omit_boundary, 0, s.halo, lr=0.02, capacity=300, blur_sigma=3.0)
        losses = loop.run(300, resident=resident)
        runs.append((loop.last_run_mode, loop.theta.cpu().numpy(), losses.cpu().numpy()))
    assert [r[0] for r in runs] == ["resident", "pipeline"]
    np.testing.assert_allclose(runs[0][1], runs[1][1], atol=5e-3)
    np.testing.assert_allclose(runs[0][2], runs[1][2], rtol=1e-4)
    np.testing.assert_allclose(-runs[0][1], v, atol=0.75)
    # grid + refine start (no warm start): 8 x 8 over +-12 px, then Adam
    cfg_g = dict(cfg, parameters={"trans_x": {"min": -12, "max": 12}, "trans_y": {"min": -12, "max": 12}},
                 optimizer={"method": "grid", "n_iter": 64, "refine_iters": 200, "parameters": {"lr": 0.02}})
    sg = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg_g)
    fg = sg.estimate(ev)
    assert np.all(np.abs(fg[:, 0, 0] - v) < 0.75), fg[:, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["dense-flow", "2d-translation"])
def test_estimate_survives_a_torn_resident_launch(model, monkeypatch):
    """A resident launch that ends with mixed verdicts leaves theta and the optimiser state partly written (``ResidentStateTorn``).
    ``estimate`` holds the state the window started with: it rebuilds the loop and solves the window with the four launches, as
    ``WindowPipeline`` does -- same flow as a run that never tried the resident launch."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver import fused_loop

    h, w = 96, 128
    ev = moving_points(h, w, 600, 40, np.array([2.0, -1.5]), seed=4)
    cfg = load_cfg()["solver"]
    cfg.update(motion_model=model, patch={"size": [24, 32], "sliding_window": [24, 32]},
               optimizer={"method": "Adam", "n_iter": 25, "parameters": {"lr": 0.05}},
               cost_with_weight={"image_variance": 1.0}, iwe={"method": "bilinear_vote", "blur_sigma": 0})
    ref_solver = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=dict(cfg, optimizer=dict(cfg["optimizer"], resident=False)))
    ref_solver.resident = False
    ref = ref_solver.estimate(ev)
    assert ref_solver.loop_mode == "pipeline"
    cls = fused_loop.FusedPatchLoop if model == "dense-flow" else fused_loop.Fused2dofLoop
    calls = []

    def torn(self, n_iter, spin_timeout_s=2.0):
        calls.append(n_iter)
        self.theta.add_(123.0)   # "partly written"
        raise fused_loop.ResidentStateTorn("resident launch ended with two different verdicts among its workgroups (injected)")

    monkeypatch.setattr(cls, "run_resident", torn)
    s = ebos.solver.collections["cmax"]((h, w), (h, w), solver_config=cfg)
    flow = s.estimate(ev)
    assert calls == [25] and s.loop_mode == "pipeline" and len(s.history) == 25
    np.testing.assert_array_equal(flow, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,patch,pad,omit,contrast", [
    ((96, 128), 20_000, (24, 32), 2, False, "variance"),     # 12 tiles of 32 x 32: every tile touches the border
    ((96, 128), 20_000, (24, 32), 3, True, "blur3"),         # pad 3: quads straddle the image's edge
    ((260, 346), 100_000, (20, 20), 1, True, "variance"),    # partial last tiles, W + 2 pad no multiple of 4
    ((260, 346), 100_000, (20, 20), 5, False, "blur1"),
    ((260, 346), 100_000, (20, 20), 2, True, "gm"),
    ((720, 1280), 400_000, (24, 32), 4, False, "variance"),  # 256 tiles of 45 x 80
    ((720, 1280), 400_000, (24, 32), 2, True, "gm"),
    ((720, 640), 300_000, (24, 32), 3, False, "blur3"),      # 230 tiles of 32 x 64
])
def test_resident_patch_loop_with_outer_padding(size, n_ev, patch, pad, omit, contrast):
    """``outer_padding > 0`` (src/event_image_converter.py:29-34) INSIDE the one-launch loop: every window reaches at
    least the padding ring and the border tiles own it -- publish its pixels, count their squares.  Against the four launches on the
    same padded problem: the image bit for bit, the first step's loss / gradient and 40 iterations to rounding, for all three
    contrasts; events near the border so that the ring is really hit."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

    h, w = size
    rs = np.random.RandomState(23)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    a, b, c = n_ev // 6, n_ev // 3, n_ev // 2
    ev[:a, 0] = rs.randint(0, 3, a)                              # crowd the top rows / left columns / bottom rows: their taps land in the ring
    ev[a:b, 1] = rs.randint(0, 3, b - a)
    ev[b:c, 0] = h - 1 - rs.randint(0, 3, c - b)
    ev = ev[np.argsort(ev[:, 2], kind="stable")]
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="compact")
    gh, gw = ebos.solver.patch_grid_shape((h, w), patch, patch)
    theta0 = torch.from_numpy(rs.uniform(-3, 3, (2, gh, gw))).float()
    n_iter = 40
    w_var, w_gm, sigma = (0.0, 1.0, 0.0) if contrast == "gm" else (1.0, 0.0, {"variance": 0.0, "blur1": 1.0, "blur3": 3.0}[contrast])

    def make():
        return FusedPatchLoop(plan, patch, patch, theta0, w_var, 0.001, 0.01, omit, pad, "auto", lr=0.02, capacity=n_iter + 20,
                              w_gradient_magnitude=w_gm, blur_sigma=sigma)

    ref, res = make(), make()
    assert res.resident_supported(), ebos.load_library().ebos_last_error()
    l1_ref = ref.run(1, resident=False).cpu().numpy()
    l1_res = res.run(1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.resident_status == 0 and res.resident_iterations == 1
    assert ref.iwe.shape == (h + 2 * pad, w + 2 * pad)
    ring = torch.ones_like(ref.iwe, dtype=torch.bool)
    ring[pad:-pad, pad:-pad] = False
    assert float(ref.iwe[ring].abs().sum()) > 0                     # (the ring holds mass: the test exercises it)
    assert torch.equal(ref.iwe, res.iwe)                            # the padded image: same bits, ring included
    np.testing.assert_allclose(l1_res, l1_ref, rtol=1e-6)
    np.testing.assert_allclose(res.d_theta.cpu().numpy(), ref.d_theta.cpu().numpy(), rtol=1e-4, atol=1e-8)
    l_ref = ref.run(n_iter - 1, resident=False).cpu().numpy()
    l_res = res.run(n_iter - 1, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.t == n_iter
    print("max rel loss deviation", np.abs(l_res / l_ref - 1).max(), "theta", (res.theta - ref.theta).abs().max().item())
    np.testing.assert_allclose(l_res, l_ref, rtol=2e-5)
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), rtol=0, atol=5e-3)
    np.testing.assert_allclose(res.variance.cpu().numpy(), ref.variance.cpu().numpy(), rtol=2e-5)
    if contrast != "gm":   # (the variance's moments: mean and pixel count of the padded image; the gradient magnitude has none)
        assert torch.equal(ref.moments[:, 1], res.moments[:, 1]) and float(res.moments[0, 1]) == (h + 2 * pad - 2 * omit) * (w + 2 * pad - 2 * omit)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n_ev,pad,omit,sigma,frac", [((60, 78), 9_000, 2, False, 3.0, False), ((60, 78), 9_000, 1, True, 0.0, True),
                                                          ((260, 346), 100_000, 3, False, 3.0, False), ((720, 1280), 300_000, 5, True, 1.0, True)])
def test_resident_2dof_loop_with_outer_padding(size, n_ev, pad, omit, sigma, frac):
    """The 2-DoF Adam loop with ``outer_padding`` as one resident launch: the four launches' trajectory (losses to 1e-6, theta to
    1e-4 px), for integer and fractional source coordinates, with and without the blur."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import Fused2dofLoop

    h, w = size
    rs = np.random.RandomState(29)
    ev = np.stack([rs.randint(0, h, n_ev), rs.randint(0, w, n_ev), np.sort(rs.uniform(0, 0.5, n_ev)), rs.randint(0, 2, n_ev)], 1).astype(np.float64)
    a, b = n_ev // 5, n_ev // 3
    ev[:a, 0] = rs.randint(0, 2, a)
    ev[a:b, 1] = w - 1 - rs.randint(0, 2, b - a)
    if frac:
        ev[:, :2] = np.clip(ev[:, :2] + rs.uniform(-0.45, 0.45, (n_ev, 2)), 0, [h - 1, w - 1])
    ev = ev[np.argsort(ev[:, 2], kind="stable")]
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto", emit="full" if frac else "compact")
    n_iter = 40

    def make():
        return Fused2dofLoop(plan, torch.tensor([1.5, -1.0]), 1.0, omit, pad, "auto", lr=0.05, capacity=n_iter + 4, blur_sigma=sigma)

    ref, res = make(), make()
    assert res.resident_supported(), ebos.load_library().ebos_last_error()
    l_ref = ref.run(n_iter, resident=False).cpu().numpy()
    l_res = res.run(n_iter, resident=True).cpu().numpy()
    assert res.last_run_mode == "resident" and res.resident_status == 0
    assert torch.equal(ref.iwe, res.iwe) or float((ref.iwe - res.iwe).abs().max()) <= 1e-5 * float(ref.iwe.abs().max())
    np.testing.assert_allclose(l_res, l_ref, rtol=2e-6)
    np.testing.assert_allclose(res.theta.cpu().numpy(), ref.theta.cpu().numpy(), rtol=0, atol=1e-4)


def _scripted_resident_loop(outcomes):
    """A loop whose resident launches end as scripted ((status, iterations completed) or "torn"): ``run``'s booking without a GPU."""
    from event_based_bos_amd.solver import fused_loop

    class Loop(fused_loop._ResidentLoop):
        plan = type("Plan", (), {"device": torch.device("cpu")})()

        def __init__(self):
            self.losses, self.t = torch.arange(32, dtype=torch.float32), 0
            self.outcomes, self.launches, self.piped = list(outcomes), [], []

        def resident_supported(self):
            return True

        def run_resident(self, n_iter, spin_timeout_s=2.0):
            self.launches.append(n_iter)
            outcome = self.outcomes.pop(0)
            if outcome == "torn":
                raise fused_loop.ResidentStateTorn("resident launch ended with two different verdicts (scripted)")
            status, self.resident_iterations = outcome
            return status

        def run(self, n_iter, resident=None):
            return self._run(n_iter, resident, self._pipeline)

        def _pipeline(self, n_iter):
            self.piped.append(n_iter)
            self.t += n_iter

    return Loop()


def test_resident_run_booking(monkeypatch, caplog):
    """The resident protocol both fused loops share: a completed launch; a hand-over after k iterations (-102: the launches run the
    rest, the window is not tried again); a refusal (-104: all iterations as launches, not tried again); a torn launch, after which
    ``run_rebuilding_torn`` solves the window again on a fresh loop with the launches."""
    from event_based_bos_amd.solver import fused_loop

    monkeypatch.delenv("EBOS_RESIDENT", raising=False)
    done = _scripted_resident_loop([(0, 10)])
    assert done.run(10).tolist() == list(range(10))
    assert (done.t, done.last_run_mode, done.resident_status, done.launches, done.piped) == (10, "resident", 0, [10], [])
    assert not done._resident_refused

    handed = _scripted_resident_loop([(-102, 4)])
    assert handed.run(10).tolist() == list(range(10))
    assert (handed.t, handed.last_run_mode, handed.resident_iterations, handed.piped) == (10, "resident+pipeline", 4, [6])
    handed.run(3)
    assert (handed.t, handed.last_run_mode, handed.launches, handed.piped) == (13, "pipeline", [10], [6, 3])

    refused = _scripted_resident_loop([(-104, 0)])
    assert refused.run(10).tolist() == list(range(10))
    assert (refused.t, refused.last_run_mode, refused.resident_status, refused.piped) == (10, "pipeline", -104, [10])
    refused.run(2)
    assert refused.launches == [10] and refused.piped == [10, 2] and refused.t == 12

    with pytest.raises(ValueError, match="capacity"):
        refused.run(30)

    made = []

    def make_loop():
        made.append(_scripted_resident_loop(["torn"]))
        return made[-1]

    with caplog.at_level("WARNING"):
        loop = fused_loop.run_rebuilding_torn(make_loop, 7, None)
    assert len(made) == 2 and loop is made[1] and "re-solving the window with the four launches" in caplog.text
    assert made[0].launches == [7] and loop.launches == [] and loop.piped == [7]
    assert (loop.t, loop.last_run_mode) == (7, "pipeline")


@pytest.mark.gpu
def test_resident_supported_builds_no_fraction_layout():
    """``resident_supported()`` of either loop on a fresh plan of fractional source coordinates asks ``EventPlan.fractional`` and
    launches nothing: the fraction layout is built by the first launch that reads it."""
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.fused_loop import Fused2dofLoop, FusedPatchLoop

    h, w, n = 260, 346, 50_000
    rs = np.random.RandomState(3)
    ev = np.stack([rs.uniform(0, h - 1, n), rs.uniform(0, w - 1, n), np.sort(rs.uniform(0, 0.5, n)), rs.randint(0, 2, n)], 1)
    plan = ebos.EventPlan.build(torch.from_numpy(ev).cuda(), (h, w), "first", True, tile="auto")
    assert plan.fractional and not plan.compact and plan.__dict__["_frac"] is None
    gh, gw = ebos.solver.patch_grid_shape((h, w), (20, 20), (20, 20))
    patch = FusedPatchLoop(plan, (20, 20), (20, 20), torch.zeros((2, gh, gw)), 1.0, halo="auto", capacity=4)
    two = Fused2dofLoop(plan, torch.tensor([1.0, -0.5]), 1.0, halo="auto", capacity=4)
    assert patch.resident_supported(), ebos.load_library().ebos_last_error()
    assert two.resident_supported(), ebos.load_library().ebos_last_error()
    assert plan.__dict__["_frac"] is None
    patch.run(2)
    assert patch.last_run_mode == "resident" and plan.__dict__["_frac"] is not None
    assert two.run(2).shape == (2,) and two.last_run_mode == "resident"
