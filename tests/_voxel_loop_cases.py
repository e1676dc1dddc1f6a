"""Shared cases of tests/test_gpu_voxel_loop.py (and tools/bench_voxel_loop.py's sanity check): the kink-free windows, the float64
yardsticks and the float64 Adam loop the native time-aware loop is compared with.

Yardsticks, all on the CPU in float64 through torch autograd: tests/_warp_voxel_ref.py (``iwe_voxel``, ``image_variance``),
tests/_flow_voxel_grad_ref.py (``voxel_torch``) and oracle.ebos_oracle (``upsample_patch_flow``, ``flow_norm``, ``image_gradient_tv``).

Shapes: 37 x 70 with plan tile (32, 32) -- tiles overhang both axes --, 20 000 events, T = 5 unless a case says otherwise."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _flow_voxel_grad_ref as GR  # noqa: E402
import _warp_voxel_ref as R  # noqa: E402

from oracle import ebos_oracle as O  # noqa: E402

H, W, N, T5 = 37, 70, 20_000, 5
TILE = (32, 32)
PATCH = (12, 14)
HOT_PIXEL, HOT_EXTRA = (17, 33), 3000
_cache = {}


def dev():
    return torch.device("cuda:0")


def G(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return O.rel_l2(a.astype(np.float64), b.astype(np.float64))


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def voxel_u(amp, T=T5, seed=21, shape=(H, W)):
    return cached(("vox", amp, T, seed, shape), lambda: np.random.RandomState(seed).uniform(-amp, amp, (T, 2) + tuple(shape)))


def off_the_kinks(vx, seed=41, empty_bin=None, margin=5e-4):
    """(a copy of tests/test_gpu_warp_voxel.py's) 20 000 events whose float64-warped coordinates keep ``margin`` px from every
    integer (tests/_kinks.py), drawn from 20 400 candidates: one too close is replaced by a spare, so n stays 20 000.  ``empty_bin``:
    no event's time falls into that bin."""
    def make():
        pool = O.synth_events(N + 400, H, W, seed=seed, tmin=0.0, tmax=1.0)
        pool[:, 0] += np.random.RandomState(seed + 1).uniform(0, 0.99, len(pool)) * (np.arange(len(pool)) % 2 == 0)
        if empty_bin is not None:
            T = vx.shape[0]
            inside = (pool[:, 2] >= empty_bin / T) & (pool[:, 2] < (empty_bin + 1) / T)
            pool[inside, 2] = (pool[inside, 2] + 1.0 / T) % 1.0
            pool = pool[np.argsort(pool[:, 2], kind="stable")]
        pool[0, 2], pool[-1, 2] = 0.0, 1.0                                            # the window is [0, 1] whichever events stay
        keep = np.ones(len(pool), dtype=bool)
        for _ in range(16):
            ev = np.concatenate([pool[:1], pool[1:-1][keep[1:-1]][:N - 2], pool[-1:]])
            warped = R.warp_voxel(torch.from_numpy(ev), torch.from_numpy(vx), "first", True)[0].numpy()
            near = (np.abs(warped[:, :2] - np.rint(warped[:, :2])) < margin).any(1) & (warped[:, 2] != 0.0)
            near[0] = near[-1] = False
            if not near.any():
                assert len(ev) == N
                return ev
            at = np.nonzero(keep[1:-1])[0][:N - 2][near[1:-1]] + 1
            keep[at] = False
        raise AssertionError("no kink-free window found")
    return make()


def kink_free(T=T5, empty_bin=None):
    """The kink-free window under voxel_u(6, T) (seed 41; 43 with an empty bin, as tests/test_gpu_warp_voxel.py draws them)."""
    vx = voxel_u(6.0, T)
    return cached(("kinkfree", T, empty_bin), lambda: off_the_kinks(vx, seed=41 if empty_bin is None else 43, empty_bin=empty_bin))


def with_hot_pixel(ev, vx, margin=5e-4, seed=71):
    """``ev`` plus HOT_EXTRA events on the source pixel HOT_PIXEL: times that cover all the bins, shuffled (a plan keeps the order of
    a pixel's events, so the run's bins come unsorted), fractional parts inside the pixel, each candidate kept off the kinks."""
    rs = np.random.RandomState(seed)
    T = vx.shape[0]
    out = []
    while len(out) < HOT_EXTRA:
        m = 2 * HOT_EXTRA
        cand = np.stack([HOT_PIXEL[0] + rs.uniform(0.02, 0.98, m), HOT_PIXEL[1] + rs.uniform(0.02, 0.98, m),
                         rs.uniform(0.001, 0.999, m), rs.randint(0, 2, m).astype(np.float64)], axis=1)
        probe = np.concatenate([ev[:1], cand, ev[-1:]])                               # (the window stays [0, 1])
        warped = R.warp_voxel(torch.from_numpy(probe), torch.from_numpy(vx), "first", True)[0].numpy()[1:-1]
        ok = ~(np.abs(warped[:, :2] - np.rint(warped[:, :2])) < margin).any(1)
        out += list(cand[ok])
    extra = np.stack(out[:HOT_EXTRA])
    assert all((R.time_bins(np.concatenate([[0.0], extra[:, 2], [1.0]]), T)[1:-1] == k).sum() > 100 for k in range(T))
    bins = R.time_bins(np.concatenate([[0.0], extra[:, 2], [1.0]]), T)[1:-1]
    assert (np.diff(bins) < 0).any()                                                  # not sorted by bin
    # in front of the last event: the window's first and last events stay where they are
    return np.concatenate([ev[:-1], extra, ev[-1:]])


def plan_of(ebos, ev, tile=TILE, T=T5, shape=(H, W)):
    return ebos.EventPlan.build(G(ev), shape, "first", True, tile=tile, emit="full", time_bin=T)


def ref_variance_grad(key, ev, vx, omit, pad):
    """(var, d var / d voxel) of the float64 restatement."""
    def make():
        v = torch.from_numpy(vx).clone().requires_grad_(True)
        loss = R.image_variance(R.iwe_voxel(torch.from_numpy(ev), v, "first", True, (pad, pad)), omit)
        loss.backward()
        return loss.item(), v.grad.numpy()
    return cached(("vgrad", key, omit, pad), make)


# ---------------------------------------------------------------------------------------------- the loop
def theta_start(seed=81):
    """[2, gh, gw] float32 in [0.5, 3]: every upwind branch of the voxel is stable (tests/test_gpu_warp_voxel.py)."""
    gh, gw = O.patch_grid_shape((H, W), PATCH, PATCH)
    return cached(("theta", seed), lambda: np.random.RandomState(seed).uniform(0.5, 3.0, (2, gh, gw)).astype(np.float32))


def ref_voxel(theta, scheme, clamp=None):
    dense = O.upsample_patch_flow(theta, (H, W), PATCH, PATCH)
    return dense, GR.voxel_torch(dense[None], T5, scheme, "middle", clamp)[0]


def ref_loss(theta, ev, scheme, clamp=None, w_norm=0.0, w_tv=0.0, w_var=1.0):
    """The float64 objective of the ``time_aware`` block at ``theta`` (a float64 tensor; differentiable)."""
    dense, vox = ref_voxel(theta, scheme, clamp)
    loss = -w_var * R.image_variance(R.iwe_voxel(torch.from_numpy(ev), vox, "first", True))
    if w_norm:
        loss = loss + w_norm * O.flow_norm(dense)
    if w_tv:
        loss = loss + w_tv * O.image_gradient_tv(dense, torch.ones((H, W), dtype=dense.dtype))
    return loss


def loop_events(scheme, clamp=None):
    """Kink-free under the float64 voxel of theta_start()."""
    def make():
        with torch.no_grad():
            _, vox = ref_voxel(torch.from_numpy(theta_start()).double(), scheme, clamp)
        return off_the_kinks(vox.numpy(), seed=53)
    return cached(("loop_ev", scheme, clamp), make)


def ref_value_and_grad(ev, scheme, clamp, w_norm, w_tv):
    def make():
        th = torch.from_numpy(theta_start()).double().requires_grad_(True)
        loss = ref_loss(th, ev, scheme, clamp, w_norm, w_tv)
        loss.backward()
        return loss.item(), th.grad.numpy()
    return cached(("loop_grad", scheme, clamp, w_norm, w_tv), make)


def ref_adam_losses(ev, scheme, n_iter, lr=0.05, clamp=None, w_norm=0.0, w_tv=0.0):
    """``n_iter`` iterations of torch.optim.Adam on the float64 objective from theta_start(): the losses before each update."""
    def make():
        th = torch.from_numpy(theta_start()).double().requires_grad_(True)
        opt = torch.optim.Adam([th], lr=lr)
        out = []
        for _ in range(n_iter):
            opt.zero_grad(set_to_none=True)
            loss = ref_loss(th, ev, scheme, clamp, w_norm, w_tv)
            loss.backward()
            opt.step()
            out.append(loss.item())
        return out
    return cached(("loop_adam", scheme, n_iter, lr, clamp, w_norm, w_tv), make)


def solver_config(native, n_iter=5, tile=TILE, scheme="upwind", **over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": list(PATCH), "sliding_window": list(PATCH)},
           "optimizer": {"method": "Adam", "n_iter": n_iter, "parameters": {"lr": 0.05}},
           "time_aware": {"time_bin": T5, "scheme": scheme, "t0_location": "middle"}}
    if tile is not None:
        cfg["tile"] = list(tile)
    if native is not None:
        cfg["time_aware"]["native"] = native
    cfg.update(over)
    return cfg
