"""The yardstick of tests/test_gpu_flow_voxel_grad.py: gradients of the time-aware flow with respect to the flow at t0, taken by CPU
autograd through tests/_flow_voxel_ref.py, the restatement of the reference's expressions (its slice writes into fresh tensors
differentiate), and through a torch restatement of the bilinear propagation written here (the one there is numpy only).
tests/test_flow_voxel_grad.py pins every function to gradients the reference's own autograd produced
(tests/golden/golden_flow_voxel_grad.npz, written by tests/golden/make_golden_flow_voxel_grad.py).

Everything takes and returns numpy arrays and computes on CPU tensors of the array's dtype, so the comparison with the kernels is in
the same dtype: the forward bins are bit-identical, every branch decision agrees, and the two gradients are two roundings of one sum.

The tolerance is ``4 r_D max|reference gradient of the case|`` with r_32 measured by the fixture script (the largest relative float32
against float64 difference of the reference's own gradients over its branch-stable cases) and r_64 = r_32 2^-29: 2 for two evaluations
that each lie within r of the exact value, times 2 because r is a sample and not a bound.
"""
import os

import numpy as np
import torch

import _flow_voxel_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "golden_flow_voxel_grad.npz"))
R32 = float(GOLDEN["r32"])
STEP = {"upwind": R.upwind_step, "burgers": R.burgers_step}


def tolerance(dtype, reference_gradient) -> float:
    r = R32 if np.dtype(dtype) == np.float32 else R32 * 2.0 ** -29
    return 4.0 * r * float(np.abs(reference_gradient).max())


def bilinear_torch(flow: torch.Tensor, dt: float) -> torch.Tensor:
    """One bilinear propagation of a tensor [2, H, W] (reference: :345-400), differentiable: position = pixel + flow dt, four cells
    around it from floor(. + 1e-8), the weights (1 - fx)(1 - fy), (1 - fx) fy, fx (1 - fy), fx fy paired with the cells (x1, y1),
    (x1 + 1, y1), (x1, y1 + 1), (x1 + 1, y1 + 1) in that order, votes outside the image multiplied by 0 and sent to cell 0."""
    _, H, W = flow.shape
    ii, jj = torch.meshgrid(torch.arange(H, device=flow.device), torch.arange(W, device=flow.device), indexing="ij")
    x, y = (flow[0] * dt + ii).reshape(-1), (flow[1] * dt + jj).reshape(-1)
    x1, y1 = torch.floor(x + 1e-8), torch.floor(y + 1e-8)
    fx, fy = x - x1, y - y1
    weights = [(1 - fx) * (1 - fy), (1 - fx) * fy, fx * (1 - fy), fx * fy]
    cells_x, cells_y = [x1, x1 + 1, x1, x1 + 1], [y1, y1, y1 + 1, y1 + 1]
    f0, f1 = flow[0].reshape(-1), flow[1].reshape(-1)
    cells, a0, a1 = [], [], []
    for w, cx, cy in zip(weights, cells_x, cells_y):
        inside = (0 <= cy) * (cy < W) * (0 <= cx) * (cx < H)
        cells.append(((cy + cx * W) * inside).long())
        a0.append(w * f0 * inside)
        a1.append(w * f1 * inside)
    cells = torch.cat(cells)
    zero = torch.zeros(H * W, dtype=flow.dtype, device=flow.device)
    return torch.stack([zero.scatter_add(0, cells, torch.cat(a0)), zero.scatter_add(0, cells, torch.cat(a1))]).reshape(2, H, W)


def voxel_torch(flows: torch.Tensor, time_bin: int, scheme: str, t0_location: str, clamp=None, torch_wrap: bool = False) -> torch.Tensor:
    """[B, 2, H, W] -> [B, T, 2, H, W] for the four schemes, differentiable."""
    if scheme != "bilinear":
        return R.construct(flows, time_bin, scheme, t0_location, clamp, torch_wrap=torch_wrap)
    t0 = R.t0_index(t0_location, time_bin)
    voxel = torch.stack([torch.stack([bilinear_torch(f, (t - t0) / time_bin) for t in range(time_bin)]) for f in flows])
    return voxel if clamp is None else torch.clamp(voxel, -clamp, clamp)


def _backward(fn, flows: np.ndarray, upstream: np.ndarray):
    f = torch.from_numpy(np.ascontiguousarray(flows)).requires_grad_()
    out = fn(f)
    out.backward(torch.from_numpy(np.ascontiguousarray(upstream)).to(f.dtype).reshape(out.shape))
    return out.detach().numpy(), f.grad.numpy()


def voxel_grad(flows: np.ndarray, upstream: np.ndarray, time_bin: int, scheme: str, t0_location: str, clamp=None, torch_wrap: bool = False):
    """-> (the unclamped-then-clamped voxel, d sum(upstream * voxel) / d flows), both in the flows' dtype."""
    return _backward(lambda f: voxel_torch(f, time_bin, scheme, t0_location, clamp, torch_wrap), flows, upstream)


def step_grad(scheme: str, flows: np.ndarray, upstream: np.ndarray, dt: float, dx=1, dy=1):
    """One step of [B, 2, H, W]: -> (its output, the gradient of its input)."""
    return _backward(lambda f: STEP[scheme](f, dt, dx, dy), flows, upstream)


def propagate_grad(flow: np.ndarray, upstream: np.ndarray, dt: float, method: str):
    """propagate_flow_to_voxel of [2, H, W], 'same' or 'bilinear'."""
    return _backward((lambda f: torch.clone(f)) if method == "same" else (lambda f: bilinear_torch(f, dt)), flow, upstream)
