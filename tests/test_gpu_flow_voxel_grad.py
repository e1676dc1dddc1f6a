"""GPU checks of the backward of the time-aware flow (csrc/flow_voxel_grad.hip) against tests/_flow_voxel_grad_ref.py: CPU autograd
through the restatement of the reference's expressions, which tests/test_flow_voxel_grad.py pins to the reference's own gradients.

Every comparison is in the same dtype.  The forward bins are bit-identical, so sign, tie and clamp decisions agree and the kernel's
gradient and autograd's are two roundings of one exact sum: |difference| <= 4 r_D max|reference gradient of the case| with r_32 from
the fixture (7.6e-7) and r_64 = r_32 2^-29.

Shapes: [B, 2, 37, 70] with B = 1 and 3 is two tiles wide (32 x 32 in float32, 24 x 24 in float64) with ragged edges; [1, 2, 1, 9] and
[1, 2, 9, 1] are thinner than any halo.  T = 17 'middle' and T = 9 'first' put 8 steps per direction exactly at the halo cap of the
fused route, T = 19 'middle' (9 each way) takes a launch per step.  The flows hold exact zeros (ties) and values beyond the clamp.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _flow_voxel_grad_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 37, 70), (3, 37, 70), (1, 1, 9), (1, 9, 1)]
CHAINS = [(17, "middle"), (9, "first"), (19, "middle")]
SCHEMES = ("upwind", "burgers", "same", "bilinear")
DTYPES = [np.float64, np.float32]
CLAMP = 1.5
_cache = {}


def flows(shape):
    """[B, 2, H, W] in [-3, 3] with both signs and 15 % exact zeros, float64."""
    key = ("flows",) + shape
    if key not in _cache:
        B, H, W = shape
        rs = np.random.RandomState(8100 + 1000 * B + 31 * H + W)
        f = rs.uniform(-3.0, 3.0, (B, 2, H, W))
        f[rs.uniform(size=f.shape) < 0.15] = 0.0
        f.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def upstream(shape):
    key = ("up",) + tuple(shape)
    if key not in _cache:
        g = np.random.RandomState(8200 + int(np.prod(shape)) % 977).standard_normal(tuple(shape))
        g.setflags(write=False)
        _cache[key] = g
    return _cache[key]


def reference(name, flow, dtype, T, scheme, loc, clamp, wrap=False):
    """(voxel, gradient) of the helper for a named flow, computed once."""
    key = ("ref", name, np.dtype(dtype).name, T, scheme, loc, clamp, wrap and scheme == "burgers")
    if key not in _cache:
        f = flow.astype(dtype)
        up = upstream((f.shape[0], T) + f.shape[1:]).astype(dtype)
        _cache[key] = GR.voxel_grad(f, up, T, scheme, loc, clamp, torch_wrap=wrap)
    return _cache[key]


def close(got, want, dtype, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.dtype(dtype), what
    err, tol = float(np.abs(got.astype(np.float64) - want).max()), GR.tolerance(dtype, want)
    print(f"{what}: |gpu - reference| = {err:.3e}, tolerance {tol:.3e}, max|reference| = {np.abs(want).max():.3e}")
    assert err <= tol, f"{what}: |gpu - reference| = {err:.3e} > {tol:.3e}"


def gpu_gradient(flow, dtype, T, scheme, loc, clamp, wrap=False):
    from event_based_bos_amd.flow_voxel import flow_voxel_batch

    f = torch.from_numpy(flow.astype(dtype)).cuda().requires_grad_()
    voxel = flow_voxel_batch(f, T, scheme, loc, clamp, torch_burgers_wrap=wrap)
    assert voxel.grad_fn is not None and voxel.requires_grad
    voxel.backward(torch.from_numpy(upstream(tuple(voxel.shape)).astype(dtype)).cuda())
    return voxel.detach(), f.grad


@pytest.mark.parametrize("clamp", [None, CLAMP])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_voxel_gradient_is_autograds(scheme, dtype, clamp):
    for shape in SHAPES:
        for T, loc in CHAINS:
            name = "rand" + "x".join(map(str, shape))
            want_voxel, want = reference(name, flows(shape), dtype, T, scheme, loc, clamp)
            voxel, got = gpu_gradient(flows(shape), dtype, T, scheme, loc, clamp)
            if clamp is not None and shape[1] > 1:
                assert (np.abs(reference(name, flows(shape), dtype, T, scheme, loc, None)[0]) > clamp).any(), "the clamp has to cut"
            if scheme != "bilinear":   # (the bilinear votes are summed in a free order)
                assert np.array_equal(voxel.cpu().numpy(), want_voxel), (shape, T, loc)
            close(got, want, dtype, f"{scheme} {np.dtype(dtype).name} clamp {clamp} {shape} T = {T} {loc}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ["upwind", "burgers"])
def test_both_routes_give_the_gradient(scheme, dtype, monkeypatch):
    from event_based_bos_amd import _hip, flow_voxel as FV

    for shape in SHAPES:
        for clamp in (None, CLAMP):
            name = "rand" + "x".join(map(str, shape))
            want = reference(name, flows(shape), dtype, 17, scheme, "middle", clamp)[1]
            got = {}
            for route in (_hip.FLOW_ROUTE_FUSED, _hip.FLOW_ROUTE_STEPS):
                monkeypatch.setattr(FV, "_FORCE_ROUTE", route)
                got[route] = gpu_gradient(flows(shape), dtype, 17, scheme, "middle", clamp)[1]
                close(got[route], want, dtype, f"{scheme} {np.dtype(dtype).name} clamp {clamp} {shape} route {route}")
            close(got[_hip.FLOW_ROUTE_FUSED], got[_hip.FLOW_ROUTE_STEPS].cpu().numpy(), dtype, f"{scheme} {shape} fused against steps")


def tie_flows():
    """A flow whose middle is an exact-zero block, and a flow that is zero except for one pixel."""
    if "ties" not in _cache:
        block = np.array(flows((1, 37, 70)))
        block[:, :, 10:30, 20:60] = 0.0
        one = np.zeros((1, 2, 37, 70))
        one[0, 0, 31, 32] = 1.0
        _cache["ties"] = {"block": block, "one": one}
    return _cache["ties"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_ties_pass_half_the_gradient_each_way(scheme, dtype):
    for name, flow in tie_flows().items():
        for T, loc in ((5, "middle"), (17, "middle"), (19, "middle")):
            want = reference(name, flow, dtype, T, scheme, loc, None)[1]
            close(gpu_gradient(flow, dtype, T, scheme, loc, None)[1], want, dtype, f"{scheme} {np.dtype(dtype).name} {name} T = {T}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_upwind_step_of_the_one_pixel_flow_gives_the_half_and_half_value(dtype):
    from event_based_bos_amd.flow_voxel import upwind_flow_to_voxel_torch

    f = torch.zeros((1, 2, 5, 5), dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device="cuda")
    f[0, 0, 2, 2] = 1.0
    f.requires_grad_()
    upwind_flow_to_voxel_torch(f, 1.0).sum().backward()
    assert f.grad[0, 0, 3, 2].item() == 1.5      # one-sided rules give 1 or 2 (tests/test_flow_voxel_grad.py)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_torch_burgers_constructors_extra_step_is_differentiated(dtype, monkeypatch):
    from event_based_bos_amd import _hip, flow_voxel as FV

    for shape in ((3, 37, 70), (1, 1, 9)):
        flow = flows(shape)
        for T, loc in ((1, "middle"), (2, "middle"), (2, "first"), (1, "first")):
            for clamp in (None, CLAMP):
                want_voxel, want = reference("rand" + "x".join(map(str, shape)), flow, dtype, T, "burgers", loc, clamp, wrap=True)
                for route in (None, _hip.FLOW_ROUTE_STEPS):
                    monkeypatch.setattr(FV, "_FORCE_ROUTE", route)
                    f = torch.from_numpy(flow.astype(dtype)).cuda().requires_grad_()
                    voxel = FV.construct_dense_flow_voxel_torch(f, T, "burgers", loc, clamp)
                    assert np.array_equal(voxel.detach().cpu().numpy(), want_voxel)
                    voxel.backward(torch.from_numpy(upstream(tuple(voxel.shape)).astype(dtype)).cuda())
                    close(f.grad, want, dtype, f"burgers wrap {np.dtype(dtype).name} {shape} T = {T} {loc} clamp {clamp} route {route}")
    # a single flow [2, H, W]: the gradient has the input's shape
    flow = flows((1, 37, 70))
    f = torch.from_numpy(flow[0].astype(dtype)).cuda().requires_grad_()
    voxel = FV.construct_dense_flow_voxel_torch(f, 2, "burgers", "middle")
    assert tuple(voxel.shape) == (2, 2, 37, 70)
    voxel.backward(torch.from_numpy(upstream((1,) + tuple(voxel.shape)).astype(dtype)).cuda()[0])
    close(f.grad, reference("rand1x37x70", flow, dtype, 2, "burgers", "middle", None, wrap=True)[1][0], dtype, "single flow")


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_functions_differentiate(dtype):
    from event_based_bos_amd import flow_voxel as FV

    fns = {"upwind": FV.upwind_flow_to_voxel_torch, "burgers": FV.inviscid_burger_flow_to_voxel_torch}
    for shape in SHAPES:
        flow = flows(shape).astype(dtype)
        up = upstream(flow.shape).astype(dtype)
        for scheme, fn in fns.items():
            for dt, dx, dy in ((0.2, 1, 1), (-0.25, 2, 4)):
                f = torch.from_numpy(flow).cuda().requires_grad_()
                out = fn(f, dt, dx, dy)
                want_out, want = GR.step_grad(scheme, flow, up, dt, dx, dy)
                assert out.grad_fn is not None and np.array_equal(out.detach().cpu().numpy(), want_out.squeeze())
                out.backward(torch.from_numpy(up).cuda().reshape(out.shape))
                close(f.grad, want, dtype, f"{scheme} step {np.dtype(dtype).name} {shape} dt = {dt}")
            f = torch.from_numpy(flow).cuda().requires_grad_()
            assert fn(f, 0.0) is f                                   # dt == 0: the input itself, so the gradient is the identity
    # a single flow [2, H, W], and a CPU tensor: the result comes back where the flow lives and the gradient reaches it
    flow = flows((1, 37, 70))[0].astype(dtype)
    up = upstream(flow.shape).astype(dtype)
    for device in ("cuda", "cpu"):
        f = torch.from_numpy(flow).to(device).requires_grad_()
        out = FV.upwind_flow_to_voxel_torch(f, -0.25, 2, 4)
        assert out.device.type == device
        out.backward(torch.from_numpy(up).to(device))
        close(f.grad, GR.step_grad("upwind", flow[None], up[None], -0.25, 2, 4)[1][0], dtype, f"single flow on {device}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_propagate_differentiates(dtype):
    from event_based_bos_amd.flow_voxel import propagate_flow_to_voxel_torch

    for shape in ((1, 37, 70), (1, 1, 9), (1, 9, 1)):
        flow = flows(shape)[0].astype(dtype)
        up = upstream(flow.shape).astype(dtype)
        for method in ("same", "bilinear"):
            for dt in (0.4, -0.7, 0.0):
                f = torch.from_numpy(flow).cuda().requires_grad_()
                out = propagate_flow_to_voxel_torch(f, dt, method)
                assert out.grad_fn is not None and tuple(out.shape) == tuple(np.squeeze(flow).shape)
                out.backward(torch.from_numpy(up).cuda().reshape(out.shape))
                want = GR.propagate_grad(flow, up, dt, method)[1]
                close(f.grad, want, dtype, f"propagate {method} {np.dtype(dtype).name} {shape} dt = {dt}")
                if dt == 0.0:
                    assert np.array_equal(f.grad.cpu().numpy(), up)  # nothing moves: the identity


@pytest.mark.parametrize("scheme", SCHEMES)
def test_gradcheck(scheme):
    from event_based_bos_amd import flow_voxel as FV

    rs = np.random.RandomState(8300)
    flow = rs.uniform(0.1, 2.0, (2, 6, 7)) * rs.choice([-1.0, 1.0], (2, 6, 7))   # |flow| > 0.1: no ties
    f = torch.from_numpy(flow).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda x: FV.construct_dense_flow_voxel_torch(x, 3, scheme, "middle"), (f,))
    if scheme in ("upwind", "burgers"):
        fn = FV.upwind_flow_to_voxel_torch if scheme == "upwind" else FV.inviscid_burger_flow_to_voxel_torch
        assert torch.autograd.gradcheck(lambda x: fn(x, -0.25, 2, 4), (f,))
    else:
        assert torch.autograd.gradcheck(lambda x: FV.propagate_flow_to_voxel_torch(x, 0.4, scheme), (f,))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_two_backward_runs_give_the_same_bits(scheme):
    for T in (17, 19):
        a = gpu_gradient(flows((3, 37, 70)), np.float32, T, scheme, "middle", CLAMP)[1]
        b = gpu_gradient(flows((3, 37, 70)), np.float32, T, scheme, "middle", CLAMP)[1]
        assert torch.equal(a, b)


def test_out_with_a_flow_that_requires_grad_and_double_backward_raise():
    from event_based_bos_amd import flow_voxel as FV

    f = torch.from_numpy(flows((1, 37, 70))).cuda().requires_grad_()
    out = torch.empty((1, 5, 2, 37, 70), dtype=torch.float64, device="cuda")
    for scheme in SCHEMES:
        with pytest.raises(ValueError, match="out="):
            FV.flow_voxel_batch(f, 5, scheme, out=out)
        FV.flow_voxel_batch(f.detach(), 5, scheme, out=out)          # without grad it is filled as before
        with torch.no_grad():
            assert FV.flow_voxel_batch(f, 5, scheme, out=out) is out
        (g,) = torch.autograd.grad(FV.flow_voxel_batch(f, 5, scheme).sum(), f, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()
    for fn in (lambda x: FV.upwind_flow_to_voxel_torch(x, 0.2), lambda x: FV.propagate_flow_to_voxel_torch(x[0], 0.2, "bilinear")):
        (g,) = torch.autograd.grad(fn(f).sum(), f, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_flow_that_does_not_require_grad_takes_the_plain_path(dtype):
    from event_based_bos_amd import flow_voxel as FV

    f = torch.from_numpy(flows((3, 37, 70)).astype(dtype)).cuda()
    for scheme in SCHEMES:
        for clamp in (None, CLAMP):
            with torch.no_grad():
                want = FV.flow_voxel_batch(f, 17, scheme, "middle", clamp)
                inside = FV.flow_voxel_batch(f.clone().requires_grad_(), 17, scheme, "middle", clamp)
            plain = FV.flow_voxel_batch(f, 17, scheme, "middle", clamp)
            tracked = FV.flow_voxel_batch(f.clone().requires_grad_(), 17, scheme, "middle", clamp)
            assert plain.grad_fn is None and not plain.requires_grad and inside.grad_fn is None and tracked.grad_fn is not None
            if scheme != "bilinear":   # (the bilinear votes are summed in a free order)
                assert torch.equal(plain, want) and torch.equal(inside, want) and torch.equal(tracked.detach(), want)
