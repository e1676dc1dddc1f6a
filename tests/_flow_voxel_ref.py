"""numpy and CPU-torch restatement of the reference's time-aware flow (src/utils/flow_utils.py:68-702), the yardstick of
tests/test_gpu_flow_voxel.py.  tests/test_flow_voxel.py pins it to arrays the reference itself produced
(tests/golden/golden_flow_voxel.npz) with ``array_equal``, and to closed forms.

Every function takes numpy arrays or CPU tensors and computes in the input's dtype with the reference's order of operations, on
shifted slices instead of the reference's diff / pad / concatenate.  Flows are [B, 2, H, W] here and come back in that shape: the
reference's final ``squeeze`` is left to the product.  flow[:, 0] moves along H, flow[:, 1] along W.
"""
import numpy as np
import torch


def _is_t(a):
    return isinstance(a, torch.Tensor)


def _zeros(a):
    return torch.zeros_like(a) if _is_t(a) else np.zeros_like(a)


def _max0(a):
    return torch.maximum(a, torch.zeros_like(a)) if _is_t(a) else np.maximum(a, 0)


def _min0(a):
    return torch.minimum(a, torch.zeros_like(a)) if _is_t(a) else np.minimum(a, 0)


def _sign(a):
    return torch.sign(a) if _is_t(a) else np.sign(a)


def _diff_back(a, axis):
    """a[i] - a[i - 1] along ``axis`` (-2 or -1), 0 at the first index."""
    d = _zeros(a)
    if axis == -2:
        d[..., 1:, :] = a[..., 1:, :] - a[..., :-1, :]
    else:
        d[..., 1:] = a[..., 1:] - a[..., :-1]
    return d


def _diff_forw(a, axis):
    """a[i + 1] - a[i] along ``axis``, 0 at the last index."""
    d = _zeros(a)
    if axis == -2:
        d[..., :-1, :] = a[..., 1:, :] - a[..., :-1, :]
    else:
        d[..., :-1] = a[..., 1:] - a[..., :-1]
    return d


def _shift(a, axis, forward):
    """a[i + 1] (forward) or a[i - 1] along ``axis`` with the edge value repeated."""
    s = a.clone() if _is_t(a) else a.copy()
    if axis == -2:
        if forward:
            s[..., :-1, :] = a[..., 1:, :]
        else:
            s[..., 1:, :] = a[..., :-1, :]
    else:
        if forward:
            s[..., :-1] = a[..., 1:]
        else:
            s[..., 1:] = a[..., :-1]
    return s


def _stack(u, v):
    return torch.stack([u, v], dim=1) if _is_t(u) else np.stack([u, v], axis=1)


def upwind_step(flow, dt, dx=1, dy=1):
    """One upwind step of [B, 2, H, W] (:447-556)."""
    if dt == 0:
        return flow
    sign, dt = (1.0 if dt > 0 else -1.0), abs(float(dt))
    f = flow * sign
    u, v = f[:, 0], f[:, 1]
    u_dx_b, u_dx_f = _diff_back(u, -2) / dx, _diff_forw(u, -2) / dx
    u_dy_b, u_dy_f = _diff_back(u, -1) / dx, _diff_forw(u, -1) / dx      # (by dx: the reference's)
    v_dx_b, v_dx_f = _diff_back(v, -2) / dy, _diff_forw(v, -2) / dy      # (by dy: the reference's)
    v_dy_b, v_dy_f = _diff_back(v, -1) / dy, _diff_forw(v, -1) / dy
    up, un, vp, vn = _max0(u), _min0(u), _max0(v), _min0(v)
    nu = u - dt * (up * u_dx_b + un * u_dx_f + vp * u_dy_b + vn * u_dy_f)
    nv = v - dt * (up * v_dx_b + un * v_dx_f + vp * v_dy_b + vn * v_dy_f)
    return _stack(nu, nv) * sign


def burgers_step(flow, dt, dx=1, dy=1):
    """One inviscid Burgers step of [B, 2, H, W] (:559-702)."""
    if dt == 0:
        return flow
    sign, dt = (1.0 if dt > 0 else -1.0), abs(float(dt))
    f = flow * sign
    u, v = f[:, 0], f[:, 1]
    u_forw, u_back = _shift(u, -2, True), _shift(u, -2, False)
    v_forw, v_back = _shift(v, -1, True), _shift(v, -1, False)
    bf_u = (u ** 2 * _sign(u) + _max0(_sign(u_back)) * (-u_back * u_back) - _min0(_sign(u_forw)) * (u_forw * u_forw)) / 2.0
    bf_v = (v ** 2 * _sign(v) + _max0(_sign(v_back)) * (-v_back * v_back) - _min0(_sign(v_forw)) * (v_forw * v_forw)) / 2.0
    u_dy_b, u_dy_f = _diff_back(u, -1) / dx, _diff_forw(u, -1) / dx
    v_dx_b, v_dx_f = _diff_back(v, -2) / dy, _diff_forw(v, -2) / dy
    up, un, vp, vn, zero = _max0(u), _min0(u), _max0(v), _min0(v), _zeros(u)
    nu = u - dt * (up * zero + un * zero + vp * u_dy_b + vn * u_dy_f + bf_u)
    nv = v - dt * (up * v_dx_b + un * v_dx_f + vp * zero + vn * zero + bf_v)
    return _stack(nu, nv) * sign


def _clip(a, c):
    return torch.clamp(a, -c, c) if _is_t(a) else np.clip(a, -c, c)


def bilinear_votes(flow, dt):
    """The twelve arrays of one bilinear propagation of [2, H, W] (:243-292): -> (cells int64 [4 n], votes of flow[0] [4 n], votes of
    flow[1] [4 n]) in the reference's order, in the flow's dtype, masked votes as value * 0 at cell 0.  numpy only."""
    _, H, W = flow.shape
    T = flow.dtype.type
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = (flow[0] * T(dt) + ii.astype(flow.dtype)).ravel()
    y = (flow[1] * T(dt) + jj.astype(flow.dtype)).ravel()
    x1, y1 = np.floor(x + T(1e-8)), np.floor(y + T(1e-8))
    fx, fy = x - x1, y - y1
    one = T(1)
    weights = [(one - fx) * (one - fy), (one - fx) * fy, fx * (one - fy), fx * fy]
    cells_x, cells_y = [x1, x1 + one, x1, x1 + one], [y1, y1, y1 + one, y1 + one]
    f0, f1 = flow[0].ravel(), flow[1].ravel()
    cells, a0, a1 = [], [], []
    for w, cx, cy in zip(weights, cells_x, cells_y):
        inside = (0 <= cy) & (cy < W) & (0 <= cx) & (cx < H)
        cells.append(np.where(inside, cx * W + cy, 0).astype(np.int64))
        a0.append((w * f0) * inside)
        a1.append((w * f1) * inside)
    return np.concatenate(cells), np.concatenate(a0), np.concatenate(a1)


def propagate_bilinear(flow, dt):
    """[2, H, W] -> (out [2, H, W] summed one vote after the other in the flow's dtype, k int64 [2, H, W] non-zero votes per cell,
    sabs float64 [2, H, W] the sum of their magnitudes): |any order of summation - out| <= 2 k u sabs.  numpy only."""
    _, H, W = flow.shape
    cells, a0, a1 = bilinear_votes(flow, dt)
    out = np.zeros((2, H * W), dtype=flow.dtype)
    k = np.zeros((2, H * W), dtype=np.int64)
    sabs = np.zeros((2, H * W), dtype=np.float64)
    for c, a in enumerate((a0, a1)):
        np.add.at(out[c], cells, a)
        np.add.at(k[c], cells, (a != 0).astype(np.int64))
        np.add.at(sabs[c], cells, np.abs(a.astype(np.float64)))
    return out.reshape(2, H, W), k.reshape(2, H, W), sabs.reshape(2, H, W)


def t0_index(t0_location, time_bin):
    return {"first": 0, "middle": time_bin // 2}[t0_location]


def construct(flows, time_bin, scheme, t0_location, clamp=None, torch_wrap=False):
    """[B, 2, H, W] -> [B, T, 2, H, W] for upwind | burgers | same (:130-146, :195-211).  torch_wrap: the torch Burgers constructor's
    backward loop, which runs down to bin 0 and stores one more step in bin -1."""
    step = {"upwind": upwind_step, "burgers": burgers_step, "same": None}[scheme]
    t0, dt = t0_index(t0_location, time_bin), 1.0 / time_bin
    bins = [None] * time_bin
    if step is None:
        bins = [flows] * time_bin
    else:
        bins[t0] = flows
        for i in range(t0, -1 if (torch_wrap and scheme == "burgers") else 0, -1):
            bins[i - 1] = step(bins[i], -dt)
        for i in range(t0, time_bin - 1):
            bins[i + 1] = step(bins[i], dt)
    voxel = torch.stack(bins, dim=1) if _is_t(flows) else np.stack(bins, axis=1)
    return voxel if clamp is None else _clip(voxel, clamp)


def construct_bilinear(flows, time_bin, t0_location, clamp=None):
    """numpy [B, 2, H, W] -> (voxel [B, T, 2, H, W], k, sabs) with dt = (bin - t0) / T per bin, each flow on its own."""
    t0 = t0_index(t0_location, time_bin)
    parts = [[propagate_bilinear(f, (t - t0) / time_bin) for t in range(time_bin)] for f in flows]
    voxel, k, sabs = (np.stack([np.stack([p[q] for p in row]) for row in parts]) for q in range(3))
    return (voxel if clamp is None else _clip(voxel, clamp)), k, sabs


def truncate_mean(voxel):
    """numpy [T, 2, H, W] -> float64 [2, H, W] (:85-90), the bins added in index order."""
    mask = (np.sqrt(voxel[:, 0] * voxel[:, 0] + voxel[:, 1] * voxel[:, 1]) > 0.0)[:, None]
    total, count = voxel[0] * mask[0], mask[0].astype(np.int64)
    for t in range(1, voxel.shape[0]):
        total = total + voxel[t] * mask[t]
        count = count + mask[t]
    return total / (count + 1e-6)
