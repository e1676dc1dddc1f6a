"""Shared cases of tests/test_gpu_hvp_tiles.py (and the per-cell pin of tests/test_hvp.py): what tests/_multiref_cases.py and
tests/_hvp_cases.py do for a fixed 37 x 70, as functions of the image shape, so that every built (tile_h, tile_w, halo) of the
second-order kernels meets a window in which it has interior tiles, four-window corners, overhang on both axes and -- for the
combine pass -- cells that several tile rows cover.

Windows, all on [0, 1], warp direction "first", every other event with a fractional row (``pool_events``), each event kept 5e-4 px
from every integer under the flow of its case (offenders are replaced, never dropped):

    main      70 x 135, 30 000 events: 2 x 3 tiles of (64, 64), 3 x 3 of (32, 64), 3 x 5 of (32, 32), 5 x 3 of (16, 64); neither W nor
              W + 2 pad is a multiple of 4.  Flows uniform(-amp, amp): amp 6 stays inside every halo >= 8, amp 12 leaves halo 8.
    empty     main without the events whose source pixel has row >= 32 and column >= 64: whole tiles of every shape are empty.
    runs      main with chosen source pixels cleared and refilled to runs of exactly 1 .. 129 events (``RUN_PIXELS``), two 300-event
              pixels in adjacent columns of one row (adjacent lanes of one wave in every tile shape: keys are row-major inside a
              tile) and one on (H - 1, W - 1), the last in-image key of the overhanging corner tile (``HOT_PIXELS``).
    tiny      13 x 21, 600 events: smaller than every tile and every halo.

Yardsticks are those of tests/_hvp_cases.py: float64 on the CPU, ``torch.autograd.functional.jvp`` / ``hvp`` of ``O.iwe_dense`` ->
optional ``O.gaussian_blur3_torch`` -> ``O.image_variance`` / ``O.gradient_magnitude``, computed once per case (``cached``)."""
import numpy as np
import torch

import _hvp_cases as C
from _hvp_cases import TWO_COSTS, as_costs, cost_key  # noqa: F401
from _multiref_cases import G, cached, dev, rel  # noqa: F401
from oracle import ebos_oracle as O

MAIN, TINY = (70, 135), (13, 21)
N_OF = {MAIN: 30_000, TINY: 600}
PATCH = (12, 14)
MARGIN = 5e-4
PLAN_TILES = ((32, 32), (64, 64), (32, 64), (16, 64))
# source pixel -> its exact run length: both sides of the owner kernel's switch at 64 (and of two of its 64-event trips), chunk tails
# of every length, spread over the tiles of every shape
RUN_PIXELS = {(3, 7): 1, (3, 8): 2, (20, 40): 3, (33, 66): 4, (40, 100): 5, (10, 63): 63, (10, 64): 64, (31, 31): 65, (50, 20): 127,
              (64, 64): 128, (69, 100): 129}
HOT_RUN = 300
HOT_PIXELS = ((45, 70), (45, 71), (MAIN[0] - 1, MAIN[1] - 1))
CONSTRUCTED = {**RUN_PIXELS, **{p: HOT_RUN for p in HOT_PIXELS}}   # pixel -> run length


def flow_u(shape, amp=6.0, seed=21):
    return cached(("t-flow", shape, amp, seed), lambda: np.random.RandomState(seed).uniform(-amp, amp, (2,) + tuple(shape)))


def direction_v(shape, seed=91):
    """A direction [2, H, W] of unit-order entries."""
    return cached(("t-v", shape, seed), lambda: np.random.RandomState(seed).standard_normal((2,) + tuple(shape)))


def pool_events(shape, n, seed=41):
    """n + n // 50 candidates on [0, 1]; every other one with a fractional row (tests/_multiref_cases.pool_events)."""
    pool = O.synth_events(n + n // 50, shape[0], shape[1], seed=seed, tmin=0.0, tmax=1.0)
    pool[:, 0] += np.random.RandomState(seed + 1).uniform(0, 0.99, len(pool)) * (np.arange(len(pool)) % 2 == 0)
    pool[0, 2], pool[-1, 2] = 0.0, 1.0                                                # the window is [0, 1] whichever events stay
    return pool


def near_kink(ev, flow, margin=MARGIN):
    """Which events lie within ``margin`` px of an integer with their float64 warped coordinates (dt == 0: exempt, zero gradient)."""
    warped = O.warp_dense_numpy(ev, flow, "first", True)
    return (np.abs(warped[:, :2] - np.rint(warped[:, :2])) < margin).any(1) & (warped[:, 2] != 0.0)


def off_the_kinks(shape, flow, seed=41):
    """N_OF[shape] events off the kinks of ``flow``: offenders are replaced by spares (tests/_multiref_cases.off_the_kinks)."""
    n = N_OF[shape]
    pool = pool_events(shape, n, seed)
    keep = np.ones(len(pool), dtype=bool)
    for _ in range(16):
        ev = np.concatenate([pool[:1], pool[1:-1][keep[1:-1]][:n - 2], pool[-1:]])
        near = near_kink(ev, flow)
        near[0] = near[-1] = False
        if not near.any():
            assert len(ev) == n
            return ev
        keep[np.nonzero(keep[1:-1])[0][:n - 2][near[1:-1]] + 1] = False
    raise AssertionError("no kink-free window found")


def kink_free(shape, amp=6.0):
    return cached(("t-kinkfree", shape, amp), lambda: off_the_kinks(shape, flow_u(shape, amp)))


def source_pixels(ev):
    return ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64)


def empty_tiles_window(amp=6.0):
    """``kink_free(MAIN)`` without the events of source rows >= 32 and columns >= 64; the first and the last event (t = 0 and 1, which
    set every dt) stay, moved out of that quarter by 32 rows if they lie in it."""
    def make():
        ev = kink_free(MAIN, amp).copy()
        for i in (0, -1):
            if ev[i, 0] >= 32 and ev[i, 1] >= 64:
                ev[i, 0] -= 32 * (int(ev[i, 0]) // 32)
        r, c = source_pixels(ev)
        out = ev[~((r >= 32) & (c >= 64))]
        assert out[0, 2] == 0.0 and out[-1, 2] == 1.0 and not near_kink(out, flow_u(MAIN, amp)).any() and len(out) < len(ev) - 5000
        return out
    return cached(("t-empty", amp), make)


def extras_on(pixel, count, ev, flow, rs):
    """``count`` events on the source pixel, times uniform on (0, 1) in no order, each off the kinks (_multiref_cases.with_hot_pixel)."""
    out = []
    while len(out) < count:
        m = 2 * count + 8
        cand = np.stack([pixel[0] + rs.uniform(0.02, 0.98, m), pixel[1] + rs.uniform(0.02, 0.98, m), rs.uniform(0.001, 0.999, m),
                         rs.randint(0, 2, m).astype(np.float64)], axis=1)
        probe = np.concatenate([ev[:1], cand, ev[-1:]])                               # (the window stays [0, 1])
        out += list(cand[~near_kink(probe, flow)[1:-1]])
    return np.stack(out[:count])


def runs_window(amp=6.0, seed=71):
    """``kink_free(MAIN)`` with the pixels of RUN_PIXELS and HOT_PIXELS cleared and refilled to their exact run lengths, the extra
    events shuffled among themselves (not sorted by time)."""
    def make():
        ev, flow, rs = kink_free(MAIN, amp), flow_u(MAIN, amp), np.random.RandomState(seed)
        wanted = CONSTRUCTED
        r, c = source_pixels(ev)
        chosen = np.zeros(len(ev), dtype=bool)
        for (pr, pc) in wanted:
            chosen |= (r == pr) & (c == pc)
        assert not chosen[0] and not chosen[-1]                                       # the events that set the window stay
        base = ev[~chosen]
        extra = np.concatenate([extras_on(p, k, base, flow, rs) for p, k in wanted.items()])
        extra = extra[rs.permutation(len(extra))]
        assert (np.diff(extra[:, 2]) < 0).any()
        out = np.concatenate([base[:-1], extra, base[-1:]])
        assert not near_kink(out, flow).any()
        return out
    return cached(("t-runs", amp, seed), make)


def constructed_mask():
    """[H, W] bool: the pixels ``runs_window`` constructs."""
    m = np.zeros(MAIN, dtype=bool)
    for p in CONSTRUCTED:
        m[p] = True
    return m


def plan_of(ebos, ev, shape, tile):
    return ebos.EventPlan.build(G(ev), shape, "first", True, tile=tile, emit="full")


# ---------------------------------------------------------------------------------------------- float64 yardsticks
def ref_contrast(ev, flow, shape, cost="image_variance", omit=False, pad=0, blur=0.0):
    iwe = O.iwe_dense(torch.from_numpy(ev), flow, shape, (pad, pad), "first", True)
    if blur:
        iwe = O.gaussian_blur3_torch(iwe, blur)
    total = 0.0
    for name, wgt in as_costs(cost).items():
        total = total + wgt * (O.image_variance if name == "image_variance" else O.gradient_magnitude)(iwe, omit, "maximize")
    return total


def ref_hvp(key, ev, flow, v, cost="image_variance", omit=False, pad=0, blur=0.0):
    """(value, gradient [2, H, W], Hessian-vector product [2, H, W]) by torch autograd in float64, once per case."""
    shape = tuple(flow.shape[1:])

    def make():
        fn = lambda f: ref_contrast(ev, f, shape, cost, omit, pad, blur)   # noqa: E731
        f = torch.from_numpy(flow).clone().requires_grad_(True)
        value = fn(f)
        (grad,) = torch.autograd.grad(value, f)
        _, hv = torch.autograd.functional.hvp(fn, torch.from_numpy(flow), torch.from_numpy(v))
        return value.item(), grad.numpy(), hv.numpy()
    return cached(("t-hvp", key, shape, hash(flow.tobytes()), hash(v.tobytes()), cost_key(cost), omit, pad, blur), make)


def ref_images(key, ev, flow, v, pad=0):
    """(IWE, tangent image) [h, w] float64: the image and its directional derivative along v by torch autograd, once per case."""
    shape = tuple(flow.shape[1:])

    def make():
        fn = lambda f: O.iwe_dense(torch.from_numpy(ev), f, shape, (pad, pad), "first", True)   # noqa: E731
        iwe, tangent = torch.autograd.functional.jvp(fn, torch.from_numpy(flow), torch.from_numpy(v))
        return iwe.numpy(), tangent.numpy()
    return cached(("t-jvp", key, shape, hash(flow.tobytes()), hash(v.tobytes()), pad), make)


def per_cell(got, want):
    """max |got - want| / max |want|: the per-cell form of a relative bar (a slip in one seam row or one corner cell fails alone)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / np.abs(want).max())


def float32_cpu_deviation(amp=6.0):
    """What float32 arithmetic alone does to the per-cell form on the main window: ``closed_form`` in float32 on the CPU against the
    float64 yardsticks -> {"iwe", "tangent", "d_flow", "hv"}: per-cell deviations (pad 0, variance contrast)."""
    def make():
        ev, flow, v = kink_free(MAIN, amp), flow_u(MAIN, amp), direction_v(MAIN)
        iwe, tangent = ref_images(("kf", amp), ev, flow, v, 0)
        _, grad, hv = ref_hvp(("kf", amp), ev, flow, v)
        _, g32, hv32, i32, t32 = C.closed_form(ev, flow, v, dtype=torch.float32, shape=MAIN)
        return {"iwe": per_cell(i32, iwe), "tangent": per_cell(t32, tangent), "d_flow": per_cell(g32, grad), "hv": per_cell(hv32, hv)}
    return cached(("t-f32", amp), make)


# ---------------------------------------------------------------------------------------------- the solver
def theta_start(shape=MAIN, seed=81):
    gh, gw = O.patch_grid_shape(shape, PATCH, PATCH)
    return cached(("t-theta", shape, seed), lambda: np.random.RandomState(seed).uniform(0.5, 3.0, (2, gh, gw)).astype(np.float32))


def dense_of(theta, shape=MAIN):
    return O.upsample_patch_flow(theta, shape, PATCH, PATCH)


def solver_events(shape=MAIN):
    """Kink-free under the float64 dense flow of theta_start()."""
    def make():
        with torch.no_grad():
            dense = dense_of(torch.from_numpy(theta_start(shape)).double(), shape).numpy()
        return off_the_kinks(shape, dense, seed=53)
    return cached(("t-solver-ev", shape), make)


def ref_loss(theta, ev, shape=MAIN):
    """The float64 loss of the solver with the variance contrast alone at ``theta`` (a float64 tensor; differentiable twice)."""
    return -ref_contrast(ev, dense_of(theta, shape), shape)


def ref_loss_hvp(ev, p, shape=MAIN):
    """(loss, gradient, product with p) of ``ref_loss`` at theta_start(), float64."""
    def make():
        fn = lambda t: ref_loss(t, ev, shape)   # noqa: E731
        th = torch.from_numpy(theta_start(shape)).double().requires_grad_(True)
        loss = fn(th)
        (grad,) = torch.autograd.grad(loss, th)
        _, hv = torch.autograd.functional.hvp(fn, torch.from_numpy(theta_start(shape)).double(), torch.from_numpy(p).double())
        return loss.item(), grad.numpy(), hv.numpy()
    return cached(("t-loss-hvp", shape, p.tobytes()), make)


def solver_config(method="Newton-CG", n_iter=4, tile=None, **over):
    """``tile=None``: no ``tile`` key -- the solver's own choice."""
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": list(PATCH), "sliding_window": list(PATCH)}, "optimizer": {"method": method, "n_iter": n_iter}}
    if tile is not None:
        cfg["tile"] = list(tile)
    cfg.update(over)
    return cfg
