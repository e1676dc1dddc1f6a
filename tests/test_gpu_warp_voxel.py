"""GPU tests of the time-aware warp (csrc/warp_voxel.hip): the materialised warp bit for bit against tests/_warp_voxel_ref.py (which
tests/test_warp_voxel.py pins to the reference by composition), the fused IWE and its backward against the float64 restatement and CPU
autograd at the project's bars (IWE relative L2 < 1e-4, contrast < 1e-5, flow gradients relative L2 < 1e-3; float64 API gradients
< 1e-10), the chain flow -> voxel -> contrast -> gradient, and the solver's ``time_aware`` block.

Gradient comparisons keep the events off the kinks of the vote (tests/_kinks.py explains why): candidates whose float64-warped
coordinate lies within 5e-4 px of an integer are replaced by spare ones, so n stays 20 000."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _flow_voxel_grad_ref as GR  # noqa: E402
import _warp_voxel_ref as R  # noqa: E402

from oracle import ebos_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "golden_warp_voxel.npz"))
DIRECTIONS = ("first", "middle", "last", 0.3, "before", "after")
BINS = (1, 2, 3, 5)
H, W, N, T5 = 37, 70, 20_000, 5
_cache = {}


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


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


# ---------------------------------------------------------------------------------------------- materialised warp
def small_voxel(T, b):
    """[b, T, 2, 5, 7] float64, every bin's flow different."""
    return np.random.RandomState(600 + 10 * T + b).uniform(-1.5, 1.5, (b, T, 2, 5, 7))


def as_container(a, kind, dtype):
    a = a.astype(dtype)
    return a if kind == "numpy" else (torch.from_numpy(a) if kind == "cpu" else G(a))


def to_numpy(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("T", BINS)
def test_warp_voxel_is_bit_identical_to_the_restatement(ebos, dtype, b, T):
    """Image 5 x 7, n = 200, times with tmin, tmax and exact bin boundaries (the fixture's events); every direction, normalize_t on and
    off, numpy / CPU-tensor / GPU-tensor containers."""
    vx = small_voxel(T, b)
    for window in ("unit", "sec"):
        ev = GOLD[f"ev_{window}_{b}"]
        for norm in (False, True):
            wp = ebos.Warp((5, 7), normalize_t=norm)
            for d, direction in enumerate(DIRECTIONS):
                want = R.warp_voxel(torch.from_numpy(ev.astype(dtype)), torch.from_numpy(vx.astype(dtype)), direction, norm).numpy()
                want = want.squeeze()                                  # the reference's .squeeze() of the result
                for kind in (("numpy", "cpu", "gpu") if d % 2 == 0 else ("gpu",)):
                    e, v = as_container(ev, kind, dtype), as_container(vx, kind, dtype)
                    if b == 1:
                        e, v = e[0], v[0]
                    got, feat = wp.warp_event(e, v, "dense-flow-voxel", direction)
                    assert type(got) is type(e) and isinstance(feat, dict)
                    if kind == "gpu":
                        assert got.is_cuda
                    got = to_numpy(got)
                    assert got.dtype == want.dtype and got.shape == want.shape
                    assert np.array_equal(got, want), (window, norm, direction, kind)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_one_bin_is_bit_identical_to_dense_flow_and_the_explicit_reference_time_entry(ebos, dtype):
    ev2, vx2 = G(GOLD["ev_sec_2"], dtype), G(small_voxel(1, 2), dtype)
    for norm in (False, True):
        wp = ebos.Warp((5, 7), normalize_t=norm, strict=True)
        for direction in DIRECTIONS:
            assert torch.equal(wp.warp_event(ev2, vx2, "dense-flow-voxel", direction)[0], wp.warp_event(ev2, vx2[:, 0], "dense-flow", direction)[0])
            assert torch.equal(wp.warp_event(ev2[0], vx2[0], "dense-flow-voxel", direction)[0],
                               wp.warp_event(ev2[0], vx2[0, 0], "dense-flow", direction)[0])
    # an explicit reference time: dt from it, the bins from the window's own time range
    ev, vx = GOLD["ev_sec_1"][0], small_voxel(3, 1)[0]
    wp = ebos.Warp((5, 7), normalize_t=False)
    got, _ = wp.warp_event_from_optical_flow_voxel(ev, vx, 1.25)
    want = R.warp_voxel(torch.from_numpy(ev), torch.from_numpy(vx), ref=torch.tensor(1.25, dtype=torch.float64)).numpy()[0]
    assert np.array_equal(got, want)
    assert np.array_equal(to_numpy(ebos.time_bins(G(GOLD["ev_sec_2"], dtype), 5)), R.time_bins(GOLD["ev_sec_2"][..., 2].astype(
        np.float32 if dtype == torch.float32 else np.float64), 5))


def test_all_times_equal_and_the_memo_and_a_foreign_bins_array(ebos):
    ev = GOLD["ev_unit_1"][0].copy()
    ev[:, 2] = 0.75
    vx = small_voxel(3, 1)[0]
    got, _ = ebos.Warp((5, 7)).warp_event(ev, vx, "dense-flow-voxel", "middle")
    assert np.array_equal(got[:, :2], ev[:, :2]) and (got[:, 2] == 0).all()       # dt == 0: nothing moves; every event in bin 0
    assert (to_numpy(ebos.time_bins(G(ev)[None], 3)) == 0).all()
    # the time-range memo on the caller's tensor, as for dense-flow
    e = G(GOLD["ev_sec_1"][0])
    wp = ebos.Warp((5, 7))
    a, _ = wp.warp_event(e, G(vx), "dense-flow-voxel")
    assert e._ebos_time_range[0] == e._version
    b, _ = wp.warp_event(e, G(vx), "dense-flow-voxel")
    assert torch.equal(a, b) and getattr(a, "_ebos_provenance", None) is None and type(a) is torch.Tensor
    # bins made for more bins than the voxel has are read as min(bin, T - 1): never outside the voxel
    e3 = e[None]
    bins9 = ebos.time_bins(e3, 9)
    out = ebos.warp_voxel(e3, G(vx)[None], 0, 0.0, False, 7, None, None, None, bins9)
    want = ebos.warp_voxel(e3, G(vx)[None], 0, 0.0, False, 7, None, None, None, torch.clamp(bins9, max=2))
    assert torch.equal(out, want)


def test_out_of_range_source_pixel_raises_under_strict(ebos):
    ev = GOLD["ev_sec_1"][0].copy()
    ev[7, 0] = 6.0                                                                 # row 6 of a 5-row flow field
    vx = small_voxel(3, 1)[0]
    with pytest.raises(IndexError):
        ebos.Warp((5, 7), strict=True).warp_event(G(ev), G(vx), "dense-flow-voxel")
    with pytest.raises(IndexError):
        ebos.Warp((5, 7)).warp_event(ev, vx, "dense-flow-voxel")                    # numpy: immediate by default, as dense-flow
    wp = ebos.Warp((5, 7))                                                          # GPU tensors: deferred, as dense-flow
    out, _ = wp.warp_event(G(ev), G(vx), "dense-flow-voxel")
    assert torch.equal(out[7, :2].cpu(), torch.tensor([6.0, ev[7, 1]], dtype=torch.float64))   # passed through un-displaced
    with pytest.raises(IndexError):
        wp.check_out_of_range()


@pytest.mark.parametrize("b", [1, 2])
def test_warp_voxel_backward_is_cpu_autograd_fp64(ebos, b):
    ev, vx = GOLD[f"ev_sec_{b}"], small_voxel(5, b)
    up = np.random.RandomState(77).standard_normal(ev.shape)
    for norm, direction in ((False, "first"), (True, 0.3), (True, "after")):
        v_ref = torch.from_numpy(vx).clone().requires_grad_(True)
        R.warp_voxel(torch.from_numpy(ev), v_ref, direction, norm).backward(torch.from_numpy(up))
        v = G(vx).requires_grad_(True)
        e = G(ev)
        out, _ = ebos.Warp((5, 7), normalize_t=norm).warp_event(e if b == 2 else e[0], v if b == 2 else v[0], "dense-flow-voxel", direction)
        out.backward(G(up) if b == 2 else G(up)[0])
        assert v.grad.shape == v_ref.grad.shape and rel(v.grad, v_ref.grad) < 1e-10


# ---------------------------------------------------------------------------------------------- fused IWE
def events_20k(seed=11, integer=False):
    def make():
        ev = O.synth_events(N, H, W, seed=seed, tmin=0.0, tmax=1.0)
        if not integer:
            ev[:, 0] += np.random.RandomState(seed + 1).uniform(0, 0.99, N) * (np.arange(N) % 2 == 0)   # half of them fractional
        return ev
    return cached(("ev", seed, integer), make)


def voxel_u(amp, T=T5, seed=21):
    return cached(("vox", amp, T, seed), lambda: np.random.RandomState(seed).uniform(-amp, amp, (T, 2, H, W)))


def weights_20k():
    return cached("w", lambda: np.random.RandomState(31).uniform(0.2, 1.8, N))


def ref_iwe(ev_key, ev, vx_key, vx, pad, weighted):
    def make():
        w = torch.from_numpy(weights_20k()) if weighted else 1.0
        iwe = R.iwe_voxel(torch.from_numpy(ev), torch.from_numpy(vx), "first", True, (pad, pad), w)
        return iwe.numpy(), float(R.image_variance(iwe))
    return cached(("iwe", ev_key, vx_key, pad, weighted), make)


def plan_of(ebos, ev, tile, T=T5):
    return ebos.EventPlan.build(G(ev), (H, W), "first", True, tile=tile, emit="full", time_bin=T)


@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_fused_iwe_both_routes(ebos, pad, weighted):
    """37 x 70 (no multiple of any tile), plan tile (32, 32), n = 20 000, T = 5, voxel U(-6, 6) per bin."""
    ev, vx = events_20k(), voxel_u(6.0)
    iwe_ref, var_ref = ref_iwe("a", ev, "u6", vx, pad, weighted)
    plan = plan_of(ebos, ev, (32, 32))
    assert plan.n == N and plan.time_bin == T5 and plan.bins.dtype == torch.uint8 and plan.bins.shape == (N,)
    assert np.array_equal(plan.bins.cpu().numpy(), R.time_bins(ev[:, 2], T5)[plan.perm.cpu().numpy()])   # permuted like the events
    w = G(weights_20k(), torch.float32) if weighted else None
    got = {}
    for route, halo in (("general", None), ("tiled", "auto"), ("tiled 16", 16)):
        iwe = plan.iwe_voxel(G(vx, torch.float32), pad=(pad, pad), weight=w, halo=halo)
        assert iwe.shape == (H + 2 * pad, W + 2 * pad) and iwe.dtype == torch.float32
        var = float(ebos.ops.image_variance(iwe))
        print(f"{route}: IWE rel L2 {rel(iwe, iwe_ref):.3e}, contrast rel {abs(var - var_ref) / var_ref:.3e}")
        assert rel(iwe, iwe_ref) < 1e-4 and abs(var - var_ref) < 1e-5 * var_ref, route
        got[route] = iwe
    assert rel(got["tiled"], got["general"]) < 1e-4 and rel(got["tiled 16"], got["general"]) < 1e-4
    # an un-binned plan (input order) takes the general route whatever the halo
    flat = plan_of(ebos, ev, None)
    assert not flat.binned and rel(flat.iwe_voxel(G(vx, torch.float32), pad=(pad, pad), weight=w), iwe_ref) < 1e-4


def test_fused_iwe_spill_path_beyond_the_built_halo(ebos):
    """Built halo 8 with U(-20, 20): displacements up to 20 px, so a visible share of the mass leaves the LDS window and takes the
    spill path."""
    ev, vx = events_20k(), voxel_u(20.0)
    iwe_ref, var_ref = ref_iwe("a", ev, "u20", vx, 0, False)
    warped = R.warp_voxel(torch.from_numpy(ev), torch.from_numpy(vx), "first", True)[0]
    share = float(((warped[:, :2] - torch.from_numpy(ev[:, :2])).abs().max(dim=1).values > 9.0).double().mean())
    assert share > 0.05, share                                                       # these events cannot land inside tile + 8
    plan = plan_of(ebos, ev, (32, 32))
    iwe = plan.iwe_voxel(G(vx, torch.float32), halo=8)
    var = float(ebos.ops.image_variance(iwe))
    print(f"halo 8, {share:.1%} of the events beyond it: IWE rel L2 {rel(iwe, iwe_ref):.3e}, contrast rel {abs(var - var_ref) / var_ref:.3e}")
    assert rel(iwe, iwe_ref) < 1e-4 and abs(var - var_ref) < 1e-5 * var_ref
    assert rel(iwe, plan.iwe_voxel(G(vx, torch.float32), halo=None)) < 1e-4


def test_one_bin_fused_iwe_is_iwe_dense(ebos):
    ev, fl = events_20k(), voxel_u(6.0, T=1, seed=22)
    plan = plan_of(ebos, ev, (32, 32), T=1)
    assert int(plan.bins.max()) == 0
    dense = plan.iwe_dense(G(fl[0], torch.float32), pad=(2, 2))
    for halo in (None, "auto"):
        assert rel(plan.iwe_voxel(G(fl, torch.float32), pad=(2, 2), halo=halo), dense) < 1e-4
    with pytest.raises(ValueError):
        plan.iwe_voxel(G(voxel_u(6.0), torch.float32))                                # a voxel of 5 bins on a plan of 1
    with pytest.raises(ValueError):
        ebos.EventPlan.build(G(ev), (H, W), tile=(32, 32)).iwe_voxel(G(fl, torch.float32))   # a plan without bins


# ---------------------------------------------------------------------------------------------- fused backward
def off_the_kinks(vx, seed=41, empty_bin=None, margin=5e-4):
    """20 000 events whose float64-warped coordinates keep ``margin`` px from every integer (tests/_kinks.py), drawn from 20 400
    candidates: one too close is replaced by a spare, so n stays 20 000.  ``empty_bin``: no event's time falls into that bin."""
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


def ref_gradients(key, ev, vx, cost, omit, weighted, pad=0):
    def make():
        v = torch.from_numpy(vx).clone().requires_grad_(True)
        w = torch.from_numpy(weights_20k()).clone().requires_grad_(True) if weighted else 1.0
        loss = R.COSTS[cost](R.iwe_voxel(torch.from_numpy(ev), v, "first", True, (pad, pad), w), omit)
        loss.backward()
        return loss.item(), v.grad.numpy(), (w.grad.numpy() if weighted else None)
    return cached(("grad", key, cost, omit, weighted, pad), make)


@pytest.mark.parametrize("tile", [(32, 32), None], ids=["sorted", "unsorted"])
def test_fused_backward_variance_folded_and_explicit(ebos, tile):
    vx = voxel_u(6.0)
    ev = cached("ev_kinkfree", lambda: off_the_kinks(vx))
    for omit in (False, True):
        loss_ref, dv_ref, dw_ref = ref_gradients("k", ev, vx, "image_variance", omit, True)
        loss_u, dv_u, _ = ref_gradients("k", ev, vx, "image_variance", omit, False)
        plan = plan_of(ebos, ev, tile)
        # the affine fold: contrast_voxel, unit weights
        v = G(vx, torch.float32).requires_grad_(True)
        c = plan.contrast_voxel(v, "image_variance", omit)
        c.backward()
        print(f"fold omit={omit}: contrast rel {abs(c.item() - loss_u) / loss_u:.3e}, d_voxel rel L2 {rel(v.grad, dv_u):.3e}")
        assert abs(c.item() - loss_u) < 1e-5 * loss_u and v.grad.shape == (T5, 2, H, W) and rel(v.grad, dv_u) < 1e-3
        # an explicit g_image through the cost op, per-event weights
        v = G(vx, torch.float32).requires_grad_(True)
        w = G(weights_20k(), torch.float32).requires_grad_(True)
        c = ebos.ops.image_variance(plan.iwe_voxel(v, weight=w, halo=None if omit else "auto"), omit)
        c.backward()
        print(f"explicit omit={omit}: d_voxel rel L2 {rel(v.grad, dv_ref):.3e}, d_weight rel L2 {rel(w.grad, dw_ref):.3e}")
        assert abs(c.item() - loss_ref) < 1e-5 * loss_ref and rel(v.grad, dv_ref) < 1e-3 and rel(w.grad, dw_ref) < 1e-3


@pytest.mark.parametrize("omit", [False, True])
@pytest.mark.parametrize("tile", [(32, 32), None], ids=["sorted", "unsorted"])
def test_fused_backward_gradient_magnitude(ebos, tile, omit):
    vx = voxel_u(6.0)
    ev = cached("ev_kinkfree", lambda: off_the_kinks(vx))
    loss_ref, dv_ref, dw_ref = ref_gradients("k", ev, vx, "gradient_magnitude", omit, True, 2)
    plan = plan_of(ebos, ev, tile)
    v = G(vx, torch.float32).requires_grad_(True)
    w = G(weights_20k(), torch.float32).requires_grad_(True)
    c = ebos.ops.gradient_magnitude(plan.iwe_voxel(v, pad=(2, 2), weight=w), omit)
    c.backward()
    print(f"d_voxel rel L2 {rel(v.grad, dv_ref):.3e}, d_weight rel L2 {rel(w.grad, dw_ref):.3e}")
    assert abs(c.item() - loss_ref) < 1e-5 * loss_ref and rel(v.grad, dv_ref) < 1e-3 and rel(w.grad, dw_ref) < 1e-3
    loss_u, dv_u, _ = ref_gradients("k", ev, vx, "gradient_magnitude", omit, False, 2)
    v = G(vx, torch.float32).requires_grad_(True)
    c = plan.contrast_voxel(v, "gradient_magnitude", omit, pad=(2, 2))
    c.backward()
    assert abs(c.item() - loss_u) < 1e-5 * loss_u and rel(v.grad, dv_u) < 1e-3


@pytest.mark.parametrize("tile", [(32, 32), None], ids=["sorted", "unsorted"])
def test_a_bin_without_events_gets_exactly_zero_and_identical_bins_sum_to_the_dense_gradient(ebos, tile):
    vx = voxel_u(6.0)
    ev = cached("ev_empty3", lambda: off_the_kinks(vx, seed=43, empty_bin=3))
    assert not (R.time_bins(ev[:, 2], T5) == 3).any() and all((R.time_bins(ev[:, 2], T5) == k).any() for k in (0, 1, 2, 4))
    _, dv_ref, _ = ref_gradients("e3", ev, vx, "image_variance", False, False)
    plan = plan_of(ebos, ev, tile)
    v = G(vx, torch.float32).requires_grad_(True)
    plan.contrast_voxel(v, "image_variance").backward()
    assert int(torch.count_nonzero(v.grad[3])) == 0 and rel(v.grad, dv_ref) < 1e-3
    # every bin the same flow: the voxel route is the dense route, and the bins' gradients add up to the flow's
    flow = G(vx[2], torch.float32)
    same = flow[None].repeat(T5, 1, 1, 1).requires_grad_(True)
    plan.contrast_voxel(same, "image_variance").backward()
    f = flow.clone().requires_grad_(True)
    plan.contrast_dense(f, "image_variance", halo=None).backward()
    print(f"sum of the bins' gradients against d_flow: rel L2 {rel(same.grad.sum(0), f.grad):.3e}")
    assert rel(same.grad.sum(0), f.grad) < 1e-3


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("scheme", ["upwind", "burgers"])
def test_flow_to_voxel_to_contrast_gradient(ebos, scheme):
    """flow [2, 37, 70] in [0.5, 3] (every upwind branch stable) -> flow_voxel_batch(T = 5, middle) -> contrast_voxel -> backward,
    against CPU autograd through tests/_flow_voxel_ref.py in float32 for the voxel and the float64 restatement for the events."""
    flow = cached("flow_e2e", lambda: np.random.RandomState(51).uniform(0.5, 3.0, (2, H, W)).astype(np.float32))
    f_ref = torch.from_numpy(flow).clone().requires_grad_(True)
    vox_ref = GR.voxel_torch(f_ref[None], T5, scheme, "middle")[0]
    ev = cached(("ev_e2e", scheme), lambda: off_the_kinks(vox_ref.detach().double().numpy(), seed=53))
    loss_ref = R.image_variance(R.iwe_voxel(torch.from_numpy(ev), vox_ref.double(), "first", True))
    loss_ref.backward()
    plan = plan_of(ebos, ev, (32, 32))
    f = G(flow).requires_grad_(True)
    voxel = ebos.flow_voxel_batch(f[None], T5, scheme, "middle")[0]
    assert torch.equal(voxel.detach().cpu(), vox_ref.detach())                     # the voxel is the restatement's, bit for bit
    c = plan.contrast_voxel(voxel, "image_variance")
    c.backward()
    print(f"{scheme}: contrast rel {abs(c.item() - loss_ref.item()) / loss_ref.item():.3e}, d_flow rel L2 {rel(f.grad, f_ref.grad):.3e}")
    assert abs(c.item() - loss_ref.item()) < 1e-5 * loss_ref.item() and rel(f.grad, f_ref.grad) < 1e-3


# ---------------------------------------------------------------------------------------------- solver
def _config(time_aware):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": [12, 14], "sliding_window": [12, 14]}, "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}}}
    if time_aware:
        cfg["time_aware"] = {"time_bin": T5, "scheme": "upwind", "t0_location": "middle"}
    return cfg


def test_solver_time_aware_block(ebos):
    from event_based_bos_amd.solver.contrast_maximization import patch_grid_shape

    ev = events_20k(seed=61, integer=True)
    make = ebos.solver.collections["contrast_maximization"]
    slv = make((H, W), (H, W), solver_config=_config(True))
    assert slv.time_aware["time_bin"] == T5 and not slv.fused_loop and not slv.use_graph
    flow = slv.estimate(ev)
    assert flow.shape == (2, H, W) and slv.loop_mode == "autograd" and not slv.fused and not slv.graphed and len(slv.history) == 5
    # the same loop by hand over the public calls
    plan = ebos.EventPlan.build(G(ev), (H, W), "first", True, tile=slv.plan_tile(), emit="full", time_bin=T5)
    theta = torch.zeros((2,) + patch_grid_shape((H, W), (12, 14), (12, 14)), dtype=torch.float32, device=dev(), requires_grad=True)
    opt = torch.optim.Adam([theta], lr=0.05)
    history = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        dense = ebos.ops.upsample_patch_flow(theta, (12, 14), (12, 14), (H, W))
        loss = -plan.contrast_voxel(ebos.flow_voxel_batch(dense[None], T5, "upwind", "middle")[0], "image_variance", False, halo="auto")
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
    print("solver", slv.history, "by hand", history)
    assert np.allclose(slv.history, history, rtol=1e-5, atol=0.0)
    assert np.isfinite(slv.history).all() and np.isfinite(flow).all()
    # without the block: the native loop, and two instances give the same bits
    a, b = make((H, W), (H, W), solver_config=_config(False)), make((H, W), (H, W), solver_config=_config(False))
    fa, fb = a.estimate(ev), b.estimate(ev)
    assert a.time_aware is None and a.fused and a.loop_mode in ("resident", "pipeline") and a.loop_mode == b.loop_mode
    assert np.array_equal(fa, fb) and a.history == b.history
    # what the block does not cover says so
    with pytest.raises(NotImplementedError):
        make((H, W), (H, W), solver_config=dict(_config(True), motion_model="2d-translation"))
    with pytest.raises(NotImplementedError):
        ebos.solver.WindowPipeline(slv)
