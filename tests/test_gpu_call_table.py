"""Which C entry points an operator enqueues, and in which order: the multi-reference / time-aware plan operators and the four warps
of ``ContrastMaximization.objective``.  No other test pins this: values and gradients stay inside their bars when a launch is added,
dropped or swapped for its twin, the launch count and the bits a route reproduces do not.

``_hip.require_gpu`` is replaced by a proxy around the real library that notes the name of every ``*_f32`` attribute called and
forwards the call.  Shape: tests/_voxel_multiref_cases.py -- 37 x 70 with plan tile (32, 32), so tiles overhang both axes, 20 000
events, T = 5, directions (first, middle, last)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multiref_cases as C  # noqa: E402
import _voxel_multiref_cases as M  # noqa: E402
from _multiref_cases import FML, G, H, W  # noqa: E402

pytestmark = pytest.mark.gpu

VAR, AFFINE = "ebos_image_variance_f32", "ebos_image_variance_affine_f32"
LOOP_FWD, LOOP_BWD = ["ebos_iwe_dense_tiled_f32"] * 3, ["ebos_iwe_dense_bwd_f32"] * 3
FUSED_FWD, FUSED_BWD = ["ebos_iwe_dense_multiref_tiled_f32"], ["ebos_iwe_dense_multiref_owner_bwd_f32"]
SLAB_FWD, SLAB_BWD = ["ebos_iwe_dense_slab_multiref_f32"], ["ebos_iwe_dense_tiled_multiref_bwd_f32"]
VOXEL_FWD, VOXEL_BWD = ["ebos_iwe_voxel_tiled_f32"], ["ebos_iwe_voxel_bwd_f32"]
VOXEL_K_FWD, VOXEL_K_BWD = ["ebos_iwe_voxel_multiref_tiled_f32"], ["ebos_iwe_voxel_multiref_owner_bwd_f32"]


class Recorder(object):
    """The library, with the name of every ``*_f32`` entry point noted as it is called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_f32"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call

    def take(self):
        out, self.calls = self.calls, []
        return out


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


@pytest.fixture
def rec(ebos, monkeypatch):
    from event_based_bos_amd import _hip

    recorder = Recorder(_hip.require_gpu())
    monkeypatch.setattr(_hip, "require_gpu", lambda: recorder)
    return recorder


def events():
    return C.plain_window()


def dense_plan(ebos):
    return C.plan_of(ebos, events())


def voxel_plan(ebos):
    return M.plan_of(ebos, events())


def flow():
    return G(C.flow_u(6.0), torch.float32).requires_grad_(True)


def voxel():
    return G(M.voxel_u(6.0), torch.float32).requires_grad_(True)


def forward_backward(rec, make):
    """(entry points of ``make()``, entry points of the backward of its sum)."""
    rec.take()
    out = make()
    fwd = rec.take()
    out.sum().backward()
    torch.cuda.synchronize()
    return fwd, rec.take()


# ---------------------------------------------------------------------------------------------- the plan operators
DENSE_OPERATORS = {
    "iwe-loop": (lambda p, f: p.iwe_dense_multi(f, FML, fused=False), LOOP_FWD, LOOP_BWD),
    # (three windows of tile (32, 32) fit the LDS only at halo 8)
    "iwe-fused": (lambda p, f: p.iwe_dense_multi(f, FML, fused=True, halo=8), FUSED_FWD, FUSED_BWD),
    "iwe-slab": (lambda p, f: p.iwe_dense_multi(f, FML, fused="slab"), SLAB_FWD, SLAB_BWD),
    "variance-loop": (lambda p, f: p.contrast_dense_multi(f, FML, "image_variance", fused=False), LOOP_FWD + [VAR], [AFFINE] + LOOP_BWD),
    "variance-fused": (lambda p, f: p.contrast_dense_multi(f, FML, "image_variance", fused=True, halo=8), FUSED_FWD + [VAR],
                       [AFFINE] + FUSED_BWD),
    "variance-slab": (lambda p, f: p.contrast_dense_multi(f, FML, "image_variance", fused="slab"), SLAB_FWD, SLAB_BWD),
}
VOXEL_OPERATORS = {
    "iwe-voxel-multi": (lambda p, v: p.iwe_voxel_multi(v, FML), VOXEL_K_FWD, VOXEL_K_BWD),
    "variance-voxel-multi": (lambda p, v: p.contrast_voxel_multi(v, FML, "image_variance"), VOXEL_K_FWD + [VAR], [AFFINE] + VOXEL_K_BWD),
    "variance-voxel": (lambda p, v: p.contrast_voxel(v, "image_variance"), VOXEL_FWD + [VAR], [AFFINE] + VOXEL_BWD),
}


@pytest.mark.parametrize("name", list(DENSE_OPERATORS))
def test_dense_multi_operator(ebos, rec, name):
    op, want_fwd, want_bwd = DENSE_OPERATORS[name]
    plan, f = dense_plan(ebos), flow()
    fwd, bwd = forward_backward(rec, lambda: op(plan, f))
    print(f"{name}: forward {fwd}, backward {bwd}")
    assert fwd == want_fwd and bwd == want_bwd


@pytest.mark.parametrize("name", list(VOXEL_OPERATORS))
def test_voxel_operator(ebos, rec, name):
    op, want_fwd, want_bwd = VOXEL_OPERATORS[name]
    plan, v = voxel_plan(ebos), voxel()
    fwd, bwd = forward_backward(rec, lambda: op(plan, v))
    print(f"{name}: forward {fwd}, backward {bwd}")
    assert fwd == want_fwd and bwd == want_bwd


def test_value_and_grad_operators(ebos, rec):
    plan, f = dense_plan(ebos), flow().detach()
    rec.take()
    plan.variance_multi_value_and_grad(f, FML)
    got = rec.take()
    print(f"variance_multi_value_and_grad: {got}")
    assert got == SLAB_FWD + SLAB_BWD
    plan, v = voxel_plan(ebos), voxel().detach()
    rec.take()
    plan.variance_voxel_value_and_grad(v)
    got = rec.take()
    print(f"variance_voxel_value_and_grad: {got}")
    assert got == VOXEL_FWD + [VAR, AFFINE, "ebos_iwe_voxel_owner_bwd_f32"]
    plan.variance_voxel_multi_value_and_grad(v, FML)
    got = rec.take()
    print(f"variance_voxel_multi_value_and_grad: {got}")
    assert got == VOXEL_K_FWD + [VAR, AFFINE] + VOXEL_K_BWD
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the solver's objective
def solver_config(warp):
    if warp == "dense":
        return C.solver_config(None)
    if warp == "multi_reference":
        return C.solver_config(FML)
    if warp == "time_aware":
        return M.L.solver_config(False)
    return M.solver_config(False)


BLUR, BLUR_BWD = ["ebos_gauss1d_f32"] * 2, ["ebos_gauss1d_bwd_f32"] * 2            # rows, then columns
GM, GM_BWD, VAR_BWD = "ebos_gradient_magnitude_f32", "ebos_gradient_magnitude_grad_f32", "ebos_image_variance_grad_f32"
TO_VOXEL, FROM_VOXEL = ["ebos_flow_voxel_advect_f32"], ["ebos_flow_voxel_advect_adjoint_f32"]
DENSE_FWD, DENSE_BWD = ["ebos_iwe_dense_slab_f32"], ["ebos_iwe_dense_tiled_bwd_f32"]
JOB, JOB_GM = "ebos_variance_dense_job_signed_f32", "ebos_gradient_magnitude_dense_job_f32"   # value and gradient in the forward


def through_images(pre, fwd, bwd, post):
    """(forward, backward) per (blurred, both contrast costs) of a warp whose operand takes ``pre`` / ``post`` to make and to leave and
    whose images take ``fwd`` / ``bwd``: un-blurred, every cost makes its own images and the variance goes back through its affine map;
    blurred, one set of images serves the cost kernels.  The backward runs the costs in reverse."""
    return {(False, False): (pre + fwd + [VAR], [AFFINE] + bwd + post),
            (False, True): (pre + fwd + [VAR] + fwd + [GM], [GM_BWD] + bwd + [AFFINE] + bwd + post),
            (True, False): (pre + fwd + BLUR + [VAR], [VAR_BWD] + BLUR_BWD + bwd + post),
            (True, True): (pre + fwd + BLUR + [VAR, GM], [GM_BWD, VAR_BWD] + BLUR_BWD + bwd + post)}


# recorded on the commit before the four bodies of ContrastMaximization._contrast became one
OBJECTIVE = {
    # (a lean plan on a slab configuration: the un-blurred contrasts come with their gradient from one job each, nothing is left to
    # the backward)
    "dense": {**through_images([], DENSE_FWD, DENSE_BWD, []), (False, False): ([JOB], []), (False, True): ([JOB, JOB_GM], [])},
    "multi_reference": through_images([], LOOP_FWD, LOOP_BWD, []),
    "time_aware": through_images(TO_VOXEL, VOXEL_FWD, VOXEL_BWD, FROM_VOXEL),
    "time_aware-directions": through_images(TO_VOXEL, VOXEL_K_FWD, VOXEL_K_BWD, FROM_VOXEL),
}
# normalize: true -- the zero-flow image and its variance once per plan, after the operand and in front of the images
NORMALIZED = {
    "multi_reference": (LOOP_FWD[:1] + [VAR] + LOOP_FWD + [VAR], [AFFINE] + LOOP_BWD),
    "time_aware-directions": (TO_VOXEL + VOXEL_FWD + [VAR] + VOXEL_K_FWD + [VAR], [AFFINE] + VOXEL_K_BWD + FROM_VOXEL),
}


@pytest.mark.parametrize("both", [False, True], ids=["variance", "both-costs"])
@pytest.mark.parametrize("blur", [0, 1.0], ids=["sharp", "blurred"])
@pytest.mark.parametrize("warp", ["dense", "multi_reference", "time_aware", "time_aware-directions"])
def test_objective(ebos, rec, warp, blur, both):
    cfg = solver_config(warp)
    cfg["iwe"] = {"blur_sigma": blur}
    cfg["cost_with_weight"] = {"image_variance": 1.0, "gradient_magnitude": 0.5} if both else {"image_variance": 1.0}
    slv = ebos.solver.collections["contrast_maximization"]((H, W), (H, W), solver_config=cfg)
    if warp == "dense":
        plan = ebos.EventPlan.build(G(events()), (H, W), "first", True, tile=slv.plan_tile(), emit="compact")
    else:
        plan = ebos.EventPlan.build(G(events()), (H, W), "first", True, tile=slv.plan_tile(), emit="full",
                                    time_bin=M.T5 if warp.startswith("time_aware") else None)
    f = flow()
    fwd, bwd = forward_backward(rec, lambda: slv.objective(plan, f))
    print(f"{warp}, blurred {bool(blur)}, both costs {both}: forward {fwd}, backward {bwd}")
    assert f.grad is not None and bool(torch.isfinite(f.grad).all())
    assert (fwd, bwd) == OBJECTIVE[warp][(bool(blur), both)]


@pytest.mark.parametrize("warp", ["multi_reference", "time_aware-directions"])
def test_objective_normalized(ebos, rec, warp):
    """``normalize: true``: the zero-flow image of the norms is made once per plan, in front of the first objective."""
    cfg = solver_config(warp)
    cfg["multi_reference" if warp == "multi_reference" else "time_aware"]["normalize"] = True
    slv = ebos.solver.collections["contrast_maximization"]((H, W), (H, W), solver_config=cfg)
    plan = ebos.EventPlan.build(G(events()), (H, W), "first", True, tile=slv.plan_tile(), emit="full",
                                time_bin=M.T5 if warp.startswith("time_aware") else None)
    first = forward_backward(rec, lambda: slv.objective(plan, flow()))
    second = forward_backward(rec, lambda: slv.objective(plan, flow()))
    print(f"{warp}: first {first}, second {second}")
    assert first == NORMALIZED[warp] and second == OBJECTIVE[warp][(False, False)]
