"""Shared cases of tests/test_multiref.py and tests/test_gpu_multiref.py (and tools/bench_multiref.py's sanity check): the
kink-free windows and the float64 yardsticks of the multi-reference contrast.

Yardsticks, all on the CPU in float64: ``oracle.ebos_oracle.iwe_dense(events, flow, (H, W), pad, direction, True)`` per direction,
``O.image_variance`` / ``O.gradient_magnitude`` / ``O.gaussian_blur3_torch`` and torch autograd.

Shapes: 37 x 70 with plan tile (32, 32) -- tiles overhang both axes --, 20 000 events on [0, 1], every other event with a fractional
row, drawn as tests/_voxel_loop_cases.off_the_kinks draws them."""
import numpy as np
import torch

from oracle import ebos_oracle as O

H, W, N = 37, 70, 20_000
TILE = (32, 32)
PATCH = (12, 14)
HOT_PIXEL, HOT_EXTRA = (17, 33), 3000
FML = ("first", "middle", "last")
FQML = ("first", 0.25, "middle", "last")
BMA = ("before", "middle", "after")
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


def flow_u(amp, seed=21):
    return cached(("flow", amp, seed), lambda: np.random.RandomState(seed).uniform(-amp, amp, (2, H, W)))


def pool_events(seed=41):
    """20 400 candidates on [0, 1]; every other one with a fractional row."""
    pool = O.synth_events(N + 400, H, W, seed=seed, tmin=0.0, tmax=1.0)
    pool[:, 0] += np.random.RandomState(seed + 1).uniform(0, 0.99, len(pool)) * (np.arange(len(pool)) % 2 == 0)
    pool[0, 2], pool[-1, 2] = 0.0, 1.0                                                # the window is [0, 1] whichever events stay
    return pool


def near_kink(ev, flow, directions, margin=5e-4):
    """Which events lie, under ANY of the directions, within ``margin`` px of an integer with their float64 warped coordinates.  An
    event with dt_k == 0 sits on a kink with a zero gradient factor and is exempt for that direction."""
    near = np.zeros(len(ev), dtype=bool)
    for d in directions:
        warped = O.warp_dense_numpy(ev, flow, d, True)
        near |= (np.abs(warped[:, :2] - np.rint(warped[:, :2])) < margin).any(1) & (warped[:, 2] != 0.0)
    return near


def plain_window(seed=41):
    """The first 20 000 candidates as they are (forward tests: no selection)."""
    def make():
        pool = pool_events(seed)
        return np.concatenate([pool[:N - 1], pool[-1:]])
    return cached(("plain", seed), make)


def off_the_kinks(flow, directions, seed=41, margin=5e-4):
    """20 000 events that keep ``margin`` px from every integer under every direction: offenders are replaced by spares, so n stays
    20 000 and no event is left out at comparison time.  Returns (events, number of offenders replaced)."""
    pool = pool_events(seed)
    keep = np.ones(len(pool), dtype=bool)
    replaced = 0
    for _ in range(16):
        ev = np.concatenate([pool[:1], pool[1:-1][keep[1:-1]][:N - 2], pool[-1:]])
        near = near_kink(ev, flow, directions, margin)
        near[0] = near[-1] = False
        if not near.any():
            assert len(ev) == N
            return ev, replaced
        at = np.nonzero(keep[1:-1])[0][:N - 2][near[1:-1]] + 1
        keep[at] = False
        replaced += int(near.sum())
    raise AssertionError("no kink-free window found")


def kink_free(directions, amp=6.0):
    return cached(("kinkfree", tuple(directions), amp), lambda: off_the_kinks(flow_u(amp), directions)[0])


def with_hot_pixel(ev, flow, directions, margin=5e-4, seed=71):
    """``ev`` plus HOT_EXTRA events on the source pixel HOT_PIXEL, times shuffled, each candidate kept off the kinks."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < HOT_EXTRA:
        m = 2 * HOT_EXTRA
        cand = np.stack([HOT_PIXEL[0] + rs.uniform(0.02, 0.98, m), HOT_PIXEL[1] + rs.uniform(0.02, 0.98, m),
                         rs.uniform(0.001, 0.999, m), rs.randint(0, 2, m).astype(np.float64)], axis=1)
        probe = np.concatenate([ev[:1], cand, ev[-1:]])                               # (the window stays [0, 1])
        out += list(cand[~near_kink(probe, flow, directions, margin)[1:-1]])
    extra = np.stack(out[:HOT_EXTRA])
    assert (np.diff(extra[:, 2]) < 0).any()                                           # not sorted by time
    return np.concatenate([ev[:-1], extra, ev[-1:]])                                  # the first and last events stay where they are


def plan_of(ebos, ev, direction="first", tile=TILE):
    return ebos.EventPlan.build(G(ev), (H, W), direction, True, tile=tile, emit="full")


# ---------------------------------------------------------------------------------------------- float64 yardsticks
def ref_iwes(ev, flow, directions, pad=0):
    """[K, h, w] float64 (flow: numpy or a float64 tensor; differentiable in the latter)."""
    fl = torch.from_numpy(flow) if isinstance(flow, np.ndarray) else flow
    return torch.stack([O.iwe_dense(torch.from_numpy(ev), fl, (H, W), (pad, pad), d, True) for d in directions])


def ref_contrast(iwes, cost="image_variance", omit=False, blur=0.0):
    """mean over the references of the raw contrast."""
    if blur:
        iwes = O.gaussian_blur3_torch(iwes, blur)
    fn = O.image_variance if cost == "image_variance" else O.gradient_magnitude
    return torch.stack([fn(iwes[k], omit, "maximize") for k in range(iwes.shape[0])]).mean()


def ref_value_and_grad(key, ev, flow, directions, cost="image_variance", omit=False, pad=0, blur=0.0):
    def make():
        f = torch.from_numpy(flow).clone().requires_grad_(True)
        v = ref_contrast(ref_iwes(ev, f, directions, pad), cost, omit, blur)
        v.backward()
        return v.item(), f.grad.numpy()
    return cached(("vgrad", key, tuple(directions), cost, omit, pad, blur), make)


# ---------------------------------------------------------------------------------------------- the solver
def theta_start(seed=81):
    """[2, gh, gw] float32 in [0.5, 3] (tests/_voxel_loop_cases.theta_start)."""
    gh, gw = O.patch_grid_shape((H, W), PATCH, PATCH)
    return cached(("theta", seed), lambda: np.random.RandomState(seed).uniform(0.5, 3.0, (2, gh, gw)).astype(np.float32))


def dense_of(theta):
    return O.upsample_patch_flow(theta, (H, W), PATCH, PATCH)


def solver_events(directions):
    """Kink-free under the float64 dense flow of theta_start(), for every direction."""
    def make():
        with torch.no_grad():
            dense = dense_of(torch.from_numpy(theta_start()).double()).numpy()
        return off_the_kinks(dense, directions, seed=53)[0]
    return cached(("solver_ev", tuple(directions)), make)


def ref_norms(ev, costs, omit=False, blur=0.0):
    """N_c: cost c of the zero-flow IWE of the window (1 where it is 0)."""
    with torch.no_grad():
        iwe = ref_iwes(ev, np.zeros((2, H, W)), ("first",))
        out = {c: ref_contrast(iwe, c, omit, blur).item() for c in costs}
    return {c: (v if v != 0.0 else 1.0) for c, v in out.items()}


def ref_loss(theta, ev, directions, weights=None, normalize=False, blur=0.0, w_norm=0.0, w_tv=0.0):
    """The float64 loss of the ``multi_reference`` block at ``theta`` (a float64 tensor; differentiable)."""
    weights = weights or {"image_variance": 1.0}
    dense = dense_of(theta)
    norms = ref_norms(ev, weights, False, blur) if normalize else {c: 1.0 for c in weights}
    iwes = ref_iwes(ev, dense, directions)
    loss = 0.0
    for c, w in weights.items():
        loss = loss - (w / norms[c]) * ref_contrast(iwes, c, False, blur)
    if w_norm:
        loss = loss + w_norm * O.flow_norm(dense)
    if w_tv:
        loss = loss + w_tv * O.image_gradient_tv(dense, torch.ones((H, W), dtype=dense.dtype))
    return loss


def ref_loss_and_grad(ev, directions, **kw):
    def make():
        th = torch.from_numpy(theta_start()).double().requires_grad_(True)
        loss = ref_loss(th, ev, directions, **kw)
        loss.backward()
        return loss.item(), th.grad.numpy()
    return cached(("loss_grad", tuple(directions), tuple(sorted((k, str(v)) for k, v in kw.items()))), make)


def ref_adam_losses(ev, directions, n_iter, lr=0.05):
    """``n_iter`` iterations of torch.optim.Adam on the float64 loss from theta_start(): the losses before each update."""
    def make():
        th = torch.from_numpy(theta_start()).double().requires_grad_(True)
        opt = torch.optim.Adam([th], lr=lr)
        out = []
        for _ in range(n_iter):
            opt.zero_grad(set_to_none=True)
            loss = ref_loss(th, ev, directions)
            loss.backward()
            opt.step()
            out.append(loss.item())
        return out
    return cached(("adam", tuple(directions), n_iter, lr), make)


def solver_config(directions=None, n_iter=5, tile=TILE, method="Adam", **over):
    """The single-reference autograd loop (``directions=None``: no block, fused loop and graph capture off) or the block's solver."""
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": list(PATCH), "sliding_window": list(PATCH)},
           "optimizer": {"method": method, "n_iter": n_iter, "parameters": {"lr": 0.05}, "fused": False, "graph": False}}
    if tile is not None:
        cfg["tile"] = list(tile)
    if directions is not None:
        cfg["multi_reference"] = {"directions": list(directions)}
    for k, v in over.items():
        if k in ("normalize", "fused"):
            cfg["multi_reference"][k] = v
        else:
            cfg[k] = v
    return cfg
