"""Shared cases of tests/test_hvp.py and tests/test_gpu_hvp.py: the windows, the float64 yardsticks and the closed form of the
contrast's Hessian-vector product.

The windows are those of tests/_multiref_cases.py with ``directions = ("first",)``: 37 x 70 with plan tile (32, 32) -- tiles overhang
both axes --, 20 000 events on [0, 1], every other one with a fractional row, each kept 5e-4 px from every integer under the flow of
the case (offenders are replaced, so no event is left out of any comparison).

The yardstick is always ``torch.autograd.functional.hvp`` of the float64 expression ``O.iwe_dense`` -> optional
``O.gaussian_blur3_torch`` -> ``O.image_variance`` / ``O.gradient_magnitude`` on the CPU.  ``closed_form`` restates, in float64 torch,
the formula the kernels implement; tests/test_hvp.py pins it against the yardstick."""
import numpy as np
import torch

import _multiref_cases as M
from _multiref_cases import G, H, N, PATCH, TILE, W, cached, dev, rel  # noqa: F401
from oracle import ebos_oracle as O

DIRS = ("first",)
TWO_COSTS = {"image_variance": 1.0, "gradient_magnitude": 0.5}


def as_costs(cost):
    return {cost: 1.0} if isinstance(cost, str) else dict(cost)


def cost_key(cost):
    return tuple(sorted(as_costs(cost).items()))


def flow_u(amp=6.0):
    return M.flow_u(amp)


def direction_v(seed=91):
    """A direction [2, H, W] of unit-order entries."""
    return cached(("hvp-v", seed), lambda: np.random.RandomState(seed).standard_normal((2, H, W)))


def kink_free(amp=6.0):
    return M.kink_free(DIRS, amp)


def with_hot_pixel(amp=6.0):
    """``kink_free`` plus 3000 events on one source pixel, their times shuffled."""
    return cached(("hvp-hot", amp), lambda: M.with_hot_pixel(kink_free(amp), flow_u(amp), DIRS))


def theta_start():
    return M.theta_start()


def solver_events():
    return M.solver_events(DIRS)


def ref_loss(theta, ev, weights=None, blur=0.0, w_norm=0.0, w_tv=0.0):
    """The float64 loss of the solver at ``theta`` (a float64 tensor; differentiable twice)."""
    return M.ref_loss(theta, ev, DIRS, weights=weights, blur=blur, w_norm=w_norm, w_tv=w_tv)


# ---------------------------------------------------------------------------------------------- float64 yardsticks
def ref_contrast(ev, flow, cost="image_variance", omit=False, pad=0, blur=0.0):
    """sum_c w_c C_c(blur(IWE(flow))), the raw contrast (flow: a float64 tensor; differentiable twice)."""
    iwe = O.iwe_dense(torch.from_numpy(ev), flow, (H, W), (pad, pad), "first", True)
    if blur:
        iwe = O.gaussian_blur3_torch(iwe, blur)
    total = 0.0
    for name, wgt in as_costs(cost).items():
        total = total + wgt * (O.image_variance if name == "image_variance" else O.gradient_magnitude)(iwe, omit, "maximize")
    return total


def ref_hvp(key, ev, flow, v, cost="image_variance", omit=False, pad=0, blur=0.0):
    """(value, gradient [2, H, W], Hessian-vector product [2, H, W]) by torch autograd in float64, computed once per case."""
    def make():
        fn = lambda f: ref_contrast(ev, f, cost, omit, pad, blur)   # noqa: E731
        f = torch.from_numpy(flow).clone().requires_grad_(True)
        value = fn(f)
        (grad,) = torch.autograd.grad(value, f)
        _, hv = torch.autograd.functional.hvp(fn, torch.from_numpy(flow), torch.from_numpy(v))
        return value.item(), grad.numpy(), hv.numpy()
    return cached(("hvp", key, hash(v.tobytes()), cost_key(cost), omit, pad, blur), make)


def ref_images(key, ev, flow, v, pad=0):
    """(IWE, tangent image) [h, w] float64: the image and its directional derivative along v by torch autograd."""
    def make():
        fn = lambda f: O.iwe_dense(torch.from_numpy(ev), f, (H, W), (pad, pad), "first", True)   # noqa: E731
        iwe, tangent = torch.autograd.functional.jvp(fn, torch.from_numpy(flow), torch.from_numpy(v))
        return iwe.numpy(), tangent.numpy()
    return cached(("jvp", key, hash(v.tobytes()), pad), make)


def ref_loss_hvp(ev, p, **kw):
    """(loss, gradient, product with p) of ``ref_loss`` at theta_start(), float64."""
    def make():
        fn = lambda t: ref_loss(t, ev, **kw)   # noqa: E731
        th = torch.from_numpy(theta_start()).double().requires_grad_(True)
        loss = fn(th)
        (grad,) = torch.autograd.grad(loss, th)
        _, hv = torch.autograd.functional.hvp(fn, torch.from_numpy(theta_start()).double(), torch.from_numpy(p).double())
        return loss.item(), grad.numpy(), hv.numpy()
    return cached(("loss-hvp", p.tobytes(), tuple(sorted((k, str(v)) for k, v in kw.items()))), make)


# ---------------------------------------------------------------------------------------------- the closed form
def _grad_map(img, cost, omit, blur):
    """The gradient map of sum_c w_c C_c(blur(img)) with respect to img.  The costs are quadratic in img, so the map is linear in
    it: at the tangent image it is the cost's Hessian applied to that image."""
    x = img.detach().clone().requires_grad_(True)
    y = O.gaussian_blur3_torch(x, blur) if blur else x
    total = 0.0
    for name, wgt in as_costs(cost).items():
        total = total + wgt * (O.image_variance if name == "image_variance" else O.gradient_magnitude)(y, omit, "maximize")
    (g,) = torch.autograd.grad(total, x)
    return total.detach(), g


def closed_form(ev, flow, v, cost="image_variance", omit=False, pad=0, blur=0.0, dtype=torch.float64, shape=None):
    """(value, d_flow, hv, iwe, tangent) by the formula of the kernels, event by event, in ``dtype`` on the CPU (``shape``: the image
    size of the window, (H, W) of this module unless given):

        s = (trunc x, trunc y);  x' = x - dt flow[0][s];  y' = y - dt flow[1][s];  (tx, ty) = (-dt v[0][s], -dt v[1][s])
        taps (R, C) = floor((x', y') + eps), fractions (fr, fc)
        tangent weights  w00' = -(1-fc) tx - (1-fr) ty   w10' = (1-fc) tx - fr ty   w01' = -fc tx + (1-fr) ty   w11' = fc tx + fr ty
        G1 = grad cost(IWE),  G2 = grad cost(tangent)
        dx(G) = (1-fc)(G10-G00) + fc(G11-G01)    dy(G) = (1-fr)(G01-G00) + fr(G11-G10)    cross = G1_00 - G1_10 - G1_01 + G1_11
        hv[:, s] += -dt (dx(G2) + cross ty, dy(G2) + cross tx)        d_flow[:, s] += -dt (dx(G1), dy(G1))"""
    H, W = shape or (M.H, M.W)
    e = torch.from_numpy(ev).to(dtype)
    fl, vv = torch.from_numpy(flow).to(dtype), torch.from_numpy(v).to(dtype)
    h, w = H + 2 * pad, W + 2 * pad
    x, y = e[:, 0], e[:, 1]
    dt = O.delta_t(torch.from_numpy(ev), O.reference_time(torch.from_numpy(ev), "first"), True).to(dtype)
    s = x.long() * W + y.long()
    f0, f1 = fl[0].reshape(-1)[s], fl[1].reshape(-1)[s]
    tx, ty = -dt * vv[0].reshape(-1)[s], -dt * vv[1].reshape(-1)[s]
    xw, yw = x - dt * f0, y - dt * f1
    r0, c0 = torch.floor(xw + O.EPS_TORCH), torch.floor(yw + O.EPS_TORCH)
    fr, fc = xw - r0, yw - c0
    R, C = r0.long() + pad, c0.long() + pad
    taps = [(R, C), (R + 1, C), (R, C + 1), (R + 1, C + 1)]                             # 00, 10, 01, 11
    inside = [((r >= 0) & (r < h) & (c >= 0) & (c < w)) for r, c in taps]
    lin = [torch.where(m, r * w + c, torch.zeros_like(r)) for (r, c), m in zip(taps, inside)]
    a, b = 1 - fr, 1 - fc

    def splat(weights):
        img = torch.zeros(h * w, dtype=dtype)
        for wgt, at, m in zip(weights, lin, inside):
            img.index_add_(0, at, wgt * m)
        return img.reshape(h, w)

    iwe = splat([a * b, fr * b, a * fc, fr * fc])
    tangent = splat([-b * tx - a * ty, b * tx - fr * ty, -fc * tx + a * ty, fc * tx + fr * ty])
    value, g1 = _grad_map(iwe, cost, omit, blur)
    _, g2 = _grad_map(tangent, cost, omit, blur)

    def gather(g):
        flat = g.reshape(-1)
        return [flat[at] * m for at, m in zip(lin, inside)]

    p, q = gather(g1), gather(g2)
    dx = lambda t: b * (t[1] - t[0]) + fc * (t[3] - t[2])   # noqa: E731
    dy = lambda t: a * (t[2] - t[0]) + fr * (t[3] - t[1])   # noqa: E731
    cross = p[0] - p[1] - p[2] + p[3]
    hv, d_flow = torch.zeros((2, H * W), dtype=dtype), torch.zeros((2, H * W), dtype=dtype)
    hv[0].index_add_(0, s, -dt * (dx(q) + cross * ty))
    hv[1].index_add_(0, s, -dt * (dy(q) + cross * tx))
    d_flow[0].index_add_(0, s, -dt * dx(p))
    d_flow[1].index_add_(0, s, -dt * dy(p))
    return value.item(), d_flow.reshape(2, H, W).numpy(), hv.reshape(2, H, W).numpy(), iwe.numpy(), tangent.numpy()


# ---------------------------------------------------------------------------------------------- the solver
def solver_config(method="Newton-CG", n_iter=5, tile=TILE, **over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": list(PATCH), "sliding_window": list(PATCH)},
           "optimizer": {"method": method, "n_iter": n_iter}}
    if tile is not None:
        cfg["tile"] = list(tile)
    cfg.update(over)
    return cfg
