"""Shared cases of tests/test_gpu_voxel_multiref.py and tests/test_gpu_voxel_multiref_loop.py: windows that are kink-free under EVERY
reference time of a case, the float64 yardsticks of the K-reference time-aware objective and its float64 Adam loop.

The yardsticks are those of tests/_voxel_loop_cases.py (imported, not copied) composed once per direction:
``_warp_voxel_ref.iwe_voxel(ev, voxel, direction_k, True, pad)`` with ``image_variance``, ``_flow_voxel_grad_ref.voxel_torch`` and the
oracle's ``upsample_patch_flow`` / ``flow_norm`` / ``image_gradient_tv``.

Shapes: 37 x 70 with plan tile (32, 32) -- tiles overhang both axes --, 20 000 events."""
import numpy as np
import torch

import _voxel_loop_cases as L
from _voxel_loop_cases import (G, GR, H, HOT_EXTRA, HOT_PIXEL, N, O, PATCH, R, T5, TILE, W, cached, dev, rel, theta_start,  # noqa: F401
                               voxel_u)

FML = ("first", "middle", "last")
FQML = ("first", 0.25, "middle", "last")


def _near_kink(ev, vx, directions, margin):
    """bool [n]: under some direction -- and some voxel, where ``vx`` is a list of them -- the float64-warped event lies within
    ``margin`` px of an integer (and is moved at all)."""
    near = np.zeros(len(ev), dtype=bool)
    for v in (vx if isinstance(vx, (list, tuple)) else [vx]):
        for d in directions:
            warped = R.warp_voxel(torch.from_numpy(ev), torch.from_numpy(np.ascontiguousarray(v)), d, True)[0].numpy()
            near |= (np.abs(warped[:, :2] - np.rint(warped[:, :2])) < margin).any(1) & (warped[:, 2] != 0.0)
    return near


def off_the_kinks(vx, directions, seed=41, empty_bin=None, margin=5e-4):
    """``_voxel_loop_cases.off_the_kinks`` with the candidate tested under every direction: N events from N + 400 candidates, one too
    close to a kink under ANY reference time replaced by a spare, so n stays N.  ``vx``: one voxel, or a list of voxels (the windows of a
    batch are warped each by its own)."""
    pool = O.synth_events(N + 400, H, W, seed=seed, tmin=0.0, tmax=1.0)
    pool[:, 0] += np.random.RandomState(seed + 1).uniform(0, 0.99, len(pool)) * (np.arange(len(pool)) % 2 == 0)
    if empty_bin is not None:
        T = (vx[0] if isinstance(vx, (list, tuple)) else vx).shape[0]
        inside = (pool[:, 2] >= empty_bin / T) & (pool[:, 2] < (empty_bin + 1) / T)
        pool[inside, 2] = (pool[inside, 2] + 1.0 / T) % 1.0
        pool = pool[np.argsort(pool[:, 2], kind="stable")]
    pool[0, 2], pool[-1, 2] = 0.0, 1.0                                            # the window is [0, 1] whichever events stay
    keep = np.ones(len(pool), dtype=bool)
    for _ in range(16):
        ev = np.concatenate([pool[:1], pool[1:-1][keep[1:-1]][:N - 2], pool[-1:]])
        near = _near_kink(ev, vx, directions, margin)
        near[0] = near[-1] = False
        if not near.any():
            assert len(ev) == N
            return ev
        at = np.nonzero(keep[1:-1])[0][:N - 2][near[1:-1]] + 1
        keep[at] = False
    raise AssertionError("no kink-free window found")


def kink_free(directions, T=T5, empty_bin=None, amp=6.0):
    """The window that is kink-free under voxel_u(amp, T) at every direction (seed 41; 43 with an empty bin)."""
    directions = tuple(directions)
    vx = voxel_u(amp, T)
    return cached(("mr_kinkfree", directions, T, empty_bin, amp),
                  lambda: off_the_kinks(vx, directions, seed=41 if empty_bin is None else 43, empty_bin=empty_bin))


def with_hot_pixel(ev, vx, directions, margin=5e-4, seed=71):
    """``_voxel_loop_cases.with_hot_pixel`` with every candidate kept off the kinks under every direction: HOT_EXTRA events on the
    source pixel HOT_PIXEL whose times cover all the bins, shuffled."""
    rs = np.random.RandomState(seed)
    T = vx.shape[0]
    out = []
    while len(out) < HOT_EXTRA:
        m = 2 * HOT_EXTRA
        cand = np.stack([HOT_PIXEL[0] + rs.uniform(0.02, 0.98, m), HOT_PIXEL[1] + rs.uniform(0.02, 0.98, m),
                         rs.uniform(0.001, 0.999, m), rs.randint(0, 2, m).astype(np.float64)], axis=1)
        probe = np.concatenate([ev[:1], cand, ev[-1:]])                               # (the window stays [0, 1])
        out += list(cand[~_near_kink(probe, vx, directions, margin)[1:-1]])
    extra = np.stack(out[:HOT_EXTRA])
    bins = R.time_bins(np.concatenate([[0.0], extra[:, 2], [1.0]]), T)[1:-1]
    assert all((bins == k).sum() > 100 for k in range(T)) and (np.diff(bins) < 0).any()   # every bin, not sorted by bin
    full = np.concatenate([ev[:-1], extra, ev[-1:]])
    assert not _near_kink(full, vx, directions, margin)[1:-1].any()
    return full


def plan_of(ebos, ev, tile=TILE, T=T5, direction="first"):
    return ebos.EventPlan.build(G(ev), (H, W), direction, True, tile=tile, emit="full", time_bin=T)


def ref_iwes(key, ev, vx, directions, pad=0):
    """float64 IWEs [K, h, w]: the restatement once per direction."""
    def make():
        with torch.no_grad():
            return torch.stack([R.iwe_voxel(torch.from_numpy(ev), torch.from_numpy(vx), d, True, (pad, pad)) for d in directions]).numpy()
    return cached(("mr_iwes", key, tuple(directions), pad), make)


def ref_mean_variance_grad(key, ev, vx, directions, omit, pad):
    """(mean_k var(IWE_k), its gradient with respect to the voxel) of the float64 restatement."""
    def make():
        v = torch.from_numpy(vx).clone().requires_grad_(True)
        loss = sum(R.image_variance(R.iwe_voxel(torch.from_numpy(ev), v, d, True, (pad, pad)), omit) for d in directions) / len(directions)
        loss.backward()
        return loss.item(), v.grad.numpy()
    return cached(("mr_vgrad", key, tuple(directions), omit, pad), make)


# ---------------------------------------------------------------------------------------------- the loop
def zero_flow_norm(ev, omit=False):
    """N of ``normalize``: the float64 variance of the window's zero-flow IWE (1 where that is 0)."""
    with torch.no_grad():
        v = R.image_variance(R.iwe_voxel(torch.from_numpy(ev), torch.zeros((1, 2, H, W), dtype=torch.float64), "first", True), omit).item()
    return v if v != 0.0 else 1.0


def ref_loss(theta, ev, directions, scheme, clamp=None, w_norm=0.0, w_tv=0.0, w_var=1.0, norm=1.0):
    """The float64 objective of the ``time_aware`` block with ``directions`` at ``theta`` (a float64 tensor; differentiable)."""
    dense, vox = L.ref_voxel(theta, scheme, clamp)
    contrast = sum(R.image_variance(R.iwe_voxel(torch.from_numpy(ev), vox, d, True)) for d in directions) / len(directions)
    loss = -(w_var / norm) * contrast
    if w_norm:
        loss = loss + w_norm * O.flow_norm(dense)
    if w_tv:
        loss = loss + w_tv * O.image_gradient_tv(dense, torch.ones((H, W), dtype=dense.dtype))
    return loss


def loop_events(directions, scheme, clamp=None):
    """Kink-free, at every direction, under the float64 voxel of theta_start()."""
    directions = tuple(directions)

    def make():
        with torch.no_grad():
            _, vox = L.ref_voxel(torch.from_numpy(theta_start()).double(), scheme, clamp)
        return off_the_kinks(vox.numpy(), directions, seed=53)
    return cached(("mr_loop_ev", directions, scheme, clamp), make)


def ref_value_and_grad(ev, directions, scheme, clamp, w_norm, w_tv, normalize):
    def make():
        th = torch.from_numpy(theta_start()).double().requires_grad_(True)
        loss = ref_loss(th, ev, directions, scheme, clamp, w_norm, w_tv, norm=zero_flow_norm(ev) if normalize else 1.0)
        loss.backward()
        return loss.item(), th.grad.numpy()
    return cached(("mr_loop_grad", tuple(directions), scheme, clamp, w_norm, w_tv, normalize), make)


def ref_adam_losses(ev, directions, scheme, n_iter, lr=0.05):
    """``n_iter`` iterations of torch.optim.Adam on the float64 objective from theta_start(): the losses before each update."""
    def make():
        th = torch.from_numpy(theta_start()).double().requires_grad_(True)
        opt = torch.optim.Adam([th], lr=lr)
        out = []
        for _ in range(n_iter):
            opt.zero_grad(set_to_none=True)
            loss = ref_loss(th, ev, directions, scheme)
            loss.backward()
            opt.step()
            out.append(loss.item())
        return out
    return cached(("mr_loop_adam", tuple(directions), scheme, n_iter, lr), make)


def solver_config(native, directions=FML, n_iter=5, tile=TILE, scheme="upwind", normalize=None, **over):
    cfg = L.solver_config(native, n_iter, tile, scheme, **over)
    cfg["time_aware"]["directions"] = list(directions)
    if normalize is not None:
        cfg["time_aware"]["normalize"] = normalize
    return cfg
