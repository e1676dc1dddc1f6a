"""GPU tests of the native time-aware loop at K reference times (``TimeAwareMultiReferencePatchLoopBatch`` and its one-window face:
``ebos_cmax_voxel_multiref_solve_batch_f32`` / ``_gradient_batch_f32``) and of the solver's ``time_aware.directions`` /
``time_aware.normalize`` keys, with and without ``native``.

Windows and yardsticks: tests/_voxel_multiref_cases.py (CPU, float64, torch autograd): 37 x 70 with plan tile (32, 32), 20 000 events
kink-free under every reference time, directions first / middle / last.  Bars are the project's: values relative < 1e-5, d_theta
relative L2 < 1e-3; five Adam iterations stay within twice the autograd loop's own distance from the float64 Adam loop."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxel_multiref_cases as M  # noqa: E402
from _voxel_multiref_cases import FML, G, H, N, PATCH, T5, W, rel  # noqa: E402

pytestmark = pytest.mark.gpu

# The native loop runs the float32 kernels of the autograd loop in another summation order: it is allowed twice the largest of the
# autograd loop's five deviations from the float64 loop, measured in the same test (the rule of tests/test_gpu_voxel_loop.py).
NATIVE_LOOP_FACTOR = 2.0


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def time_aware(scheme, clamp=None, normalize=False, directions=FML):
    return {"time_bin": T5, "scheme": scheme, "t0_location": "middle", "clamp": clamp, "native": True, "directions": list(directions),
            "normalize": normalize}


def make_loop(ebos, ev, scheme, clamp=None, w_norm=0.0, w_tv=0.0, normalize=False, capacity=8):
    from event_based_bos_amd.solver.time_aware_loop import TimeAwareMultiReferencePatchLoop

    return TimeAwareMultiReferencePatchLoop(M.plan_of(ebos, ev), PATCH, PATCH, G(M.theta_start()), time_aware(scheme, clamp, normalize), 1.0,
                                            w_norm, w_tv, lr=0.05, capacity=capacity)


# one combination per axis: both schemes, with and without the two regularisers, clamp None and 2.0, normalize on and off
@pytest.mark.parametrize("scheme,reg,clamp,normalize", [("upwind", 0.0, None, False), ("burgers", 0.1, None, True),
                                                        ("upwind", 0.1, 2.0, False), ("burgers", 0.0, 2.0, True),
                                                        ("upwind", 0.0, None, True)])
def test_loop_first_iteration_is_float64_autograd(ebos, scheme, reg, clamp, normalize):
    ev = M.loop_events(FML, scheme, clamp)
    assert len(ev) == N
    loss_ref, grad_ref = M.ref_value_and_grad(ev, FML, scheme, clamp, reg, reg, normalize)
    loop = make_loop(ebos, ev, scheme, clamp, reg, reg, normalize)
    assert loop.K == 3 and loop.iwe.shape == (1, 3, H, W) and loop.last_run_mode == "native"
    if normalize:
        n_ref = M.zero_flow_norm(ev)
        assert abs(1.0 / loop.inv_norm.item() - n_ref) < 1e-5 * n_ref
    else:
        assert loop.inv_norm.item() == 1.0
    start = loop.theta.clone()
    losses = loop.run(1)
    assert loop.t == 1 and int(loop.step.item()) == 1 and losses.shape == (1,)
    print(f"{scheme} reg={reg} clamp={clamp} normalize={normalize}: loss rel {abs(losses[0].item() - loss_ref) / abs(loss_ref):.3e}, "
          f"d_theta rel L2 {rel(loop.d_theta, grad_ref):.3e}")
    assert abs(losses[0].item() - loss_ref) < 1e-5 * abs(loss_ref) and rel(loop.d_theta, grad_ref) < 1e-3
    assert not torch.equal(loop.theta, start)                                    # Adam moved the grid
    # value_and_grad: the same kernels without the step, at the start
    value, grad = loop.value_and_grad(start)
    assert abs(value.item() - loss_ref) < 1e-5 * abs(loss_ref) and rel(grad, grad_ref) < 1e-3 and torch.equal(loop.theta, start)


def test_loop_five_iterations_follow_the_float64_adam_loop(ebos):
    ev = M.loop_events(FML, "upwind")
    want = np.array(M.ref_adam_losses(ev, FML, "upwind", 5))
    # the autograd loop of the same configuration, the same window, the same start: its own distance from the float64 loop
    slv = ebos.solver.collections["contrast_maximization"]((H, W), (H, W), solver_config=M.solver_config(None))
    slv.previous_best = M.theta_start()
    slv.estimate(ev)
    assert slv.loop_mode == "autograd" and len(slv.history) == 5
    auto = np.abs(np.array(slv.history) - want) / np.abs(want)
    print("autograd loop, deviation per iteration:", auto.tolist())
    got = make_loop(ebos, ev, "upwind").run(5).cpu().numpy().astype(np.float64)
    dev = np.abs(got - want) / np.abs(want)
    print("native loop, deviation per iteration:", dev.tolist())
    assert want[-1] < want[0] and got[-1] < got[0]                               # the loss falls
    assert (dev <= NATIVE_LOOP_FACTOR * auto.max()).all(), (dev, auto)


def events_int(seed=61):
    return M.cached(("ev_int", seed), lambda: M.O.synth_events(N, H, W, seed=seed, tmin=0.0, tmax=1.0))


def test_solver_routes_native_autograd_and_scipy(ebos):
    make = ebos.solver.collections["contrast_maximization"]
    ev = events_int()
    slv = make((H, W), (H, W), solver_config=M.solver_config(True, tile=None, normalize=True))
    assert slv.plan_tile() == (64, 64)
    flow = slv.estimate(ev)
    assert flow.shape == (2, H, W) and np.isfinite(flow).all() and np.isfinite(slv.history).all()
    assert slv.loop_mode == "native" and slv.loop_modes == ["native"] and slv.fused and not slv.graphed and len(slv.history) == 5
    # the autograd loop of the same configuration computes the same objective, with both costs and a blur too
    off = make((H, W), (H, W), solver_config=M.solver_config(False, tile=None, normalize=True))
    off.estimate(ev)
    assert off.loop_mode == "autograd" and not off.fused and len(off.history) == 5
    print("native", slv.history, "autograd", off.history)
    assert abs(off.history[0] - slv.history[0]) < 1e-5 * abs(off.history[0])
    both = M.solver_config(None, normalize=True, cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5, "flow_norm": 0.01},
                           iwe={"blur_sigma": 1})
    slv = make((H, W), (H, W), solver_config=both)
    slv.estimate(ev)
    assert slv.loop_mode == "autograd" and len(slv.history) == 5 and np.isfinite(slv.history).all()
    # a pyramid: every scale runs the native loop
    pyr = M.solver_config(True, n_iter=6)
    pyr["patch"] = {"pyramid": {"coarsest": 16, "finest": 8}}
    slv = make((H, W), (H, W), solver_config=pyr)
    slv.estimate(ev)
    assert slv.loop_modes == ["native", "native"] and len(slv.history) == sum(n for _, _, n in slv.pyramid_scales())
    # L-BFGS-B from a warm start, through value_and_grad
    cfg = M.solver_config(True)
    cfg["optimizer"] = {"method": "L-BFGS-B", "n_iter": 5}
    slv = make((H, W), (H, W), solver_config=cfg)
    slv.previous_best = M.theta_start() * 0.2
    slv.estimate(ev)
    print("L-BFGS-B", slv.history[0], "->", float(slv.scipy_result.fun), f"in {len(slv.history)} evaluations")
    assert slv.loop_mode == "native" and slv.fused and len(slv.history) >= 2 and float(slv.scipy_result.fun) < slv.history[0]


def test_estimate_is_estimate_batch_of_one_window(ebos):
    """One window is a batch of one, on one code path: ``estimate`` and ``estimate_batch`` of that window, each on its own build of the
    plan, bit for bit.  (Two builds differ in the order of the events of one source pixel; the loop reads the stack's canonical order,
    so the owner backward adds alike -- tests/test_gpu_voxel_multiref.py::test_two_builds_of_a_plan_give_the_backward_the_same_bits.)"""
    make = ebos.solver.collections["contrast_maximization"]
    ev = events_int()
    cfg = M.solver_config(True, normalize=True)
    one = make((H, W), (H, W), solver_config=cfg)
    flow = one.estimate(ev)
    batch = make((H, W), (H, W), solver_config=cfg)
    flows = batch.estimate_batch([ev])
    dev = np.abs(np.array(batch.histories[0]) - np.array(one.history)) / np.abs(np.array(one.history))
    print(f"estimate against estimate_batch of one window: flow rel L2 {rel(flows[0], flow):.3e}, history deviation {dev.tolist()}")
    assert one.loop_mode == "native" and batch.loop_mode == "native-batch" and flows.shape == (1, 2, H, W)
    assert np.array_equal(flows[0], flow) and batch.histories[0] == one.history and torch.equal(batch.patch_flows[0], one.patch_flow)
    # several windows of different sizes, in chunks: a window does not see its neighbours
    windows = [ev, np.concatenate([ev[:1], ev[1:-1][::3], ev[-1:]]), ev[ev[:, 1] < 50]]
    many = make((H, W), (H, W), solver_config=cfg)
    flows = many.estimate_batch(windows, max_batch=2)
    assert flows.shape == (3, 2, H, W) and np.isfinite(flows).all() and len(many.histories) == 3
    dev = np.abs(np.array(many.histories[0]) - np.array(one.history)) / np.abs(np.array(one.history))
    assert rel(flows[0], flow) < 1e-3 and (dev < 1e-5).all()


def test_estimate_batch_prepared_from_raw_columns(ebos, tmp_path):
    """The synthetic recording's raw columns through ``TimeAwarePlanStack.from_raw`` into the K-reference loop, against ``estimate`` on
    the same windows' event arrays (the two plans differ in the order of the events of one source pixel only)."""
    from event_based_bos_amd.evaluation import synthetic_recording, window_ingest_raw_batch

    shape = (64, 80)
    ev_path, _, _, _ = synthetic_recording(str(tmp_path / "recording"), shape, 4, 4000)
    store = ebos.RawEventStore(ev_path)
    n = len(store)
    cols = store.load_raw(0, n, device=M.dev())
    ranges = [(0, n // 2), (n // 2, n), (n // 4, 3 * n // 4)]
    prepared = window_ingest_raw_batch(cols, ranges, shape, None, None, 1e6)      # (the recording's ticks are microseconds)
    cfg = M.solver_config(True, normalize=True, tile=None)
    cfg["patch"] = {"size": [16, 20], "sliding_window": [16, 20]}
    make = ebos.solver.collections["contrast_maximization"]
    slv = make(shape, shape, solver_config=cfg)
    flows = slv.estimate_batch_prepared(prepared, max_batch=2)
    assert flows.shape == (3, 2) + shape and np.isfinite(flows).all() and slv.loop_mode == "native-batch" and len(slv.histories) == 3
    for b in range(3):
        ref = make(shape, shape, solver_config=cfg)
        want = ref.estimate(prepared.events(b).cpu().numpy())
        dev = np.abs(np.array(slv.histories[b]) - np.array(ref.history)) / np.abs(np.array(ref.history))
        print(f"window {b}: history deviation {dev.tolist()}, flow rel L2 {rel(flows[b], want):.3e}")
        assert rel(flows[b], want) < 1e-3 and (dev < 1e-5).all()
