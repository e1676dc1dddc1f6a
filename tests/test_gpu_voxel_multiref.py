"""GPU tests of the time-aware warp at K reference times: the K-image forward (``ebos_iwe_voxel_multiref_tiled[_batch]_f32``), the
K-reference pixel-owner backward (``ebos_iwe_voxel_multiref_owner_bwd[_batch]_f32``) and the plan operators over them
(``EventPlan.iwe_voxel_multi``, ``contrast_voxel_multi``, ``variance_voxel_multi_value_and_grad``).

Windows and yardsticks: tests/_voxel_multiref_cases.py -- 37 x 70 with plan tile (32, 32), 20 000 events that are kink-free under every
direction of the case; the float64 CPU restatement once per direction.  Bars are the project's, as for the single-reference voxel
kernels: IWE per reference relative L2 < 1e-4, value relative < 1e-5, d_voxel relative L2 < 1e-3."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voxel_multiref_cases as M  # noqa: E402
from _voxel_multiref_cases import FML, FQML, G, H, N, R, T5, W, rel  # noqa: E402
from _voxel_launch import GUARD, P, S, c_shifts, forward, guarded, guards_untouched, ok, owner_backward  # noqa: E402, F401

pytestmark = pytest.mark.gpu

DIRECTIONS = {1: ("last",), 3: FML, 4: FQML}


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


@pytest.fixture(scope="module")
def lib(ebos):
    from event_based_bos_amd import _hip

    return _hip.require_gpu()


def fixed_upstream(K, pad, seed=7):
    """(g_images [K, h, w], affine [K, 2]): an upstream that does not come from a forward, whose float atomics differ between runs."""
    rs = np.random.RandomState(seed)
    return G(rs.uniform(-1, 1, (K, H + 2 * pad, W + 2 * pad)), torch.float32), G(rs.uniform(0.5, 2, (K, 2)), torch.float32)


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("T", [1, 5, 255])
@pytest.mark.parametrize("K", [1, 3, 4])
def test_forward_is_the_float64_iwe_per_reference(ebos, lib, K, T, pad):
    directions = DIRECTIONS[K]
    vx, ev = M.voxel_u(6.0, T), M.kink_free(directions, T)
    assert len(ev) == N
    want = M.ref_iwes(("kf", T), ev, vx, directions, pad)
    plan = M.plan_of(ebos, ev, T=T)
    iwes = forward(lib, plan, G(vx, torch.float32), directions, 32, pad, splits=1 if pad else 3)
    for k in range(K):
        r = rel(iwes[k], want[k])
        print(f"K={K} T={T} pad={pad} reference {directions[k]!r}: IWE relative L2 {r:.3e}, mass {float(iwes[k].sum()):.1f}")
        assert r < 1e-4, (k, r)
    # the operator is the same launch
    got = plan.iwe_voxel_multi(G(vx, torch.float32), list(directions), pad=(pad, pad))
    assert got.shape == (K, H + 2 * pad, W + 2 * pad) and max(rel(got[k], want[k]) for k in range(K)) < 1e-4


@pytest.mark.parametrize("halo,built", [(8, True), (24, False)])
def test_forward_beyond_the_halo_and_without_a_built_configuration(ebos, lib, halo, built):
    """Halo 8 under displacements of up to 30 px: most events leave the LDS window and take the spill path, under ``last`` with a
    negative dt.  Halo 24 is no built configuration of tile (32, 32): the general kernel, reference by reference."""
    from event_based_bos_amd import _hip

    assert ((32, 32, halo) in set(_hip.tiled_configs())) == built
    vx, ev = M.voxel_u(30.0), M.kink_free(FML, amp=30.0)
    want = M.ref_iwes(("kf30", T5), ev, vx, FML, 0)
    plan = M.plan_of(ebos, ev)
    assert (plan.dt[:plan.n] + c_shifts(plan, FML)[0][2]).min().item() < -0.9          # `last`: dt runs down to -1
    iwes = forward(lib, plan, G(vx, torch.float32), FML, halo, 0)
    for k in range(3):
        print(f"halo {halo} reference {FML[k]!r}: IWE relative L2 {rel(iwes[k], want[k]):.3e}")
        assert rel(iwes[k], want[k]) < 1e-4, k
    got = plan.iwe_voxel_multi(G(vx, torch.float32), list(FML), halo=halo)
    assert max(rel(got[k], want[k]) for k in range(3)) < 1e-4


# ---------------------------------------------------------------------------------------------- owner backward
@pytest.mark.parametrize("omit,pad,T", [(False, 0, 5), (True, 0, 5), (False, 2, 5), (True, 2, 5), (False, 0, 255), (True, 2, 1)])
def test_owner_backward_is_float64_autograd(ebos, omit, pad, T):
    vx, ev = M.voxel_u(6.0, T), M.kink_free(FML, T)
    var_ref, dv_ref = M.ref_mean_variance_grad(("kf", T), ev, vx, FML, omit, pad)
    plan = M.plan_of(ebos, ev, T=T)
    value, d_voxel = plan.variance_voxel_multi_value_and_grad(G(vx, torch.float32), list(FML), omit, pad=(pad, pad))
    print(f"omit={omit} pad={pad} T={T}: value rel {abs(value.item() - var_ref) / var_ref:.3e}, d_voxel rel L2 {rel(d_voxel, dv_ref):.3e}")
    assert value.dim() == 0 and d_voxel.shape == (T, 2, H, W) and d_voxel.dtype == torch.float32
    assert abs(value.item() - var_ref) < 1e-5 * var_ref and rel(d_voxel, dv_ref) < 1e-3
    # upstream scales the gradient, not the value
    v2, d2 = plan.variance_voxel_multi_value_and_grad(G(vx, torch.float32), list(FML), omit, pad=(pad, pad), upstream=-0.5)
    assert torch.equal(v2, value) and rel(d2, -0.5 * dv_ref) < 1e-3


def test_owner_backward_writes_every_cell_and_is_reproducible(ebos, lib):
    vx, ev = M.voxel_u(6.0), M.kink_free(FML, empty_bin=3)
    assert not (R.time_bins(ev[:, 2], T5) == 3).any()
    _, dv_ref = M.ref_mean_variance_grad(("kf_empty3", T5), ev, vx, FML, False, 0)
    plan = M.plan_of(ebos, ev)
    out = torch.empty((T5, 2, H, W), dtype=torch.float32, device=M.dev())
    out.view(torch.uint8).fill_(0xFF)                                 # every float a NaN: a cell that is not written shows
    _, d_voxel = plan.variance_voxel_multi_value_and_grad(G(vx, torch.float32), list(FML), out=out)
    assert d_voxel.data_ptr() == out.data_ptr() and bool(torch.isfinite(out).all())
    assert int(torch.count_nonzero(out[3])) == 0 and rel(out, dv_ref) < 1e-3
    # the same inputs twice, with and without the affine maps: the order of the additions is the plan's
    for pad, g_lo in ((0, 0), (2, 1)):
        g_images, affine = fixed_upstream(3, pad)
        for aff in (affine, None):
            a = owner_backward(lib, plan, G(vx, torch.float32), FML, g_images, aff, g_lo, pad)
            b = owner_backward(lib, plan, G(vx, torch.float32), FML, g_images, aff, g_lo, pad)
            assert bool(torch.isfinite(a).all()) and int(torch.count_nonzero(a[3])) == 0 and int(torch.count_nonzero(a)) > 0
            assert torch.equal(a, b)


def test_hot_pixel_with_bins_out_of_order(ebos, lib):
    vx = M.voxel_u(6.0)
    ev = M.cached("mr_hot", lambda: M.with_hot_pixel(M.kink_free(FML), vx, FML))
    assert len(ev) == N + M.HOT_EXTRA
    var_ref, dv_ref = M.ref_mean_variance_grad(("hot", T5), ev, vx, FML, False, 0)
    plan = M.plan_of(ebos, ev)
    value, d1 = plan.variance_voxel_multi_value_and_grad(G(vx, torch.float32), list(FML))
    hot = d1[:, :, M.HOT_PIXEL[0], M.HOT_PIXEL[1]]
    print(f"hot pixel: value rel {abs(value.item() - var_ref) / var_ref:.3e}, d_voxel rel L2 {rel(d1, dv_ref):.3e}, "
          f"the hot pixel's cells rel L2 {rel(hot, dv_ref[:, :, M.HOT_PIXEL[0], M.HOT_PIXEL[1]]):.3e}")
    assert abs(value.item() - var_ref) < 1e-5 * var_ref and rel(d1, dv_ref) < 1e-3
    assert rel(hot, dv_ref[:, :, M.HOT_PIXEL[0], M.HOT_PIXEL[1]]) < 1e-3
    g_images, affine = fixed_upstream(3, 0)                            # the whole-wave walk adds in a fixed tree: the same bits twice
    a, b = (owner_backward(lib, plan, G(vx, torch.float32), FML, g_images, affine, 0, 0) for _ in range(2))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_one_reference_is_the_single_owner_backward(ebos):
    """K = 1 with the plan's own direction (shift 0: dt as it is) against ``variance_voxel_value_and_grad``."""
    vx, ev = M.voxel_u(6.0), M.kink_free(FML)
    plan = M.plan_of(ebos, ev)
    vox = G(vx, torch.float32)
    for omit, pad in ((False, 0), (True, 2)):
        v1, d1 = plan.variance_voxel_value_and_grad(vox, omit, pad=(pad, pad))
        vk, dk = plan.variance_voxel_multi_value_and_grad(vox, ["first"], omit, pad=(pad, pad))
        print(f"K=1 omit={omit} pad={pad}: value rel {abs(vk.item() - v1.item()) / v1.item():.3e}, d_voxel rel L2 {rel(dk, d1):.3e}, "
              f"bit-identical: {torch.equal(dk, d1)}")
        assert abs(vk.item() - v1.item()) < 1e-5 * v1.item() and rel(dk, d1) < 1e-3


def test_three_references_are_three_single_backwards(ebos):
    """K = 3 against the sum of three single owner backwards on plans built with each direction (upstream 1 / 3 each)."""
    vx, ev = M.voxel_u(6.0), M.kink_free(FML)
    vox = G(vx, torch.float32)
    value, d_voxel = M.plan_of(ebos, ev).variance_voxel_multi_value_and_grad(vox, list(FML), True, pad=(2, 2))
    parts = [M.plan_of(ebos, ev, direction=d).variance_voxel_value_and_grad(vox, True, pad=(2, 2), upstream=1.0 / 3.0) for d in FML]
    want_v = sum(p[0].item() for p in parts) / 3.0
    want_d = parts[0][1] + parts[1][1] + parts[2][1]
    print(f"K=3 against three single backwards: value rel {abs(value.item() - want_v) / want_v:.3e}, d_voxel rel L2 {rel(d_voxel, want_d):.3e}")
    assert abs(value.item() - want_v) < 1e-5 * want_v and rel(d_voxel, want_d) < 1e-3


def test_two_builds_of_a_plan_give_the_backward_the_same_bits(ebos, lib):
    """A plan build leaves the order of the events of one source pixel to its counting sort's atomic counter, and the owner backward
    adds in run order: on the raw streams two builds may differ in the last bits of d_voxel, on ``TimeAwarePlanStack.canonical`` (what
    the native loop reads) they cannot.  Integer-pixel events: eight to a pixel on average, so most runs hold several."""
    vx = M.voxel_u(6.0)
    ev = M.cached(("ev_int", 61), lambda: M.O.synth_events(N, H, W, seed=61, tmin=0.0, tmax=1.0))
    g_images, affine = fixed_upstream(3, 0)
    outs, raw = [], []
    for _ in range(3):
        plan = M.plan_of(ebos, ev)
        st = ebos.EventPlan.stack_time_aware([plan]).canonical()
        assert st.n == plan.n and torch.equal(st.key_offsets[0], plan.key_offsets.to(torch.int32))

        class View(object):                                       # the canonical streams under the plan's own offsets
            x, y, dt, bins, key_offsets, n, tile = st.x, st.y, st.dt, st.bins, st.key_offsets[0].contiguous(), st.n, plan.tile
            ref_fraction, normalized_t = plan.ref_fraction, plan.normalized_t

        outs.append(owner_backward(lib, View, G(vx, torch.float32), FML, g_images, affine, 0, 0))
        raw.append(owner_backward(lib, plan, G(vx, torch.float32), FML, g_images, affine, 0, 0))
        assert torch.equal(torch.sort(st.dt)[0], torch.sort(plan.dt[:plan.n])[0])       # the same events
    print("two more builds against the first, raw run order: d_voxel bit-identical", [torch.equal(raw[0], r) for r in raw[1:]],
          "rel L2", [f"{rel(r, raw[0]):.2e}" for r in raw[1:]])
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and rel(outs[0], raw[0]) < 1e-5


# ---------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("K,pad", [(3, 0), (4, 2)])
def test_iwe_voxel_multi_backward_under_a_random_upstream(ebos, K, pad):
    directions = DIRECTIONS[K]
    vx, ev = M.voxel_u(6.0), M.kink_free(directions)
    up = np.random.RandomState(5).uniform(-1, 1, (K, H + 2 * pad, W + 2 * pad))
    v64 = torch.from_numpy(vx).clone().requires_grad_(True)
    sum((R.iwe_voxel(torch.from_numpy(ev), v64, d, True, (pad, pad)) * torch.from_numpy(up[k])).sum() for k, d in enumerate(directions)).backward()
    plan = M.plan_of(ebos, ev)
    v = G(vx, torch.float32).requires_grad_(True)
    (plan.iwe_voxel_multi(v, list(directions), pad=(pad, pad)) * G(up, torch.float32)).sum().backward()
    print(f"K={K} pad={pad}: d_voxel under a random upstream, rel L2 {rel(v.grad, v64.grad):.3e}")
    assert v.grad.shape == (T5, 2, H, W) and rel(v.grad, v64.grad) < 1e-3
    # a float64 voxel gets a float64 gradient
    vd = G(vx).requires_grad_(True)
    (plan.iwe_voxel_multi(vd, list(directions), pad=(pad, pad)) * G(up)).sum().backward()
    assert vd.grad.dtype == torch.float64 and rel(vd.grad, v64.grad) < 1e-3


@pytest.mark.parametrize("cost", ["image_variance", "gradient_magnitude"])
@pytest.mark.parametrize("omit", [False, True])
def test_contrast_voxel_multi_is_float64_autograd(ebos, cost, omit):
    vx, ev = M.voxel_u(6.0), M.kink_free(FML)
    v64 = torch.from_numpy(vx).clone().requires_grad_(True)
    want = sum(R.COSTS[cost](R.iwe_voxel(torch.from_numpy(ev), v64, d, True), omit) for d in FML) / 3.0
    want.backward()
    v = G(vx, torch.float32).requires_grad_(True)
    got = M.plan_of(ebos, ev).contrast_voxel_multi(v, list(FML), cost, omit)
    got.backward()
    print(f"{cost} omit={omit}: value rel {abs(got.item() - want.item()) / want.item():.3e}, d_voxel rel L2 {rel(v.grad, v64.grad):.3e}")
    assert got.dim() == 0 and abs(got.item() - want.item()) < 1e-5 * want.item() and rel(v.grad, v64.grad) < 1e-3


# ---------------------------------------------------------------------------------------------- batch
B = 3


def batch_voxels():
    return [M.voxel_u(6.0, T5, seed=21 + b) for b in range(B)]


def batch_windows():
    """[w0, an empty window, w1]: w0 kink-free under voxels 0 and 2 at every direction, w1 its first, every third interior and last
    event (the time range, and so every kept event's bin and warp, is unchanged)."""
    def make():
        w0 = M.off_the_kinks([batch_voxels()[0], batch_voxels()[2]], FML, seed=41)
        return [w0, np.zeros((0, 4)), np.concatenate([w0[:1], w0[1:-1][::3], w0[-1:]])]
    return M.cached("mr_batch_windows", make)


class Stack3(object):
    """The stacked plan of [plans[0], an empty window, plans[1]] in the given order of slots (tests/test_gpu_voxel_loop_batch.py's
    ``WithEmpty``): an empty window's row of the offsets is constant, its base."""

    def __init__(self, ebos, plans, order):
        live = [i for i in order if i != 1]
        two = ebos.EventPlan.stack_time_aware([plans[i] for i in live])
        self.x, self.y, self.dt, self.bins, self.tile = two.x, two.y, two.dt, two.bins, two.tile
        rows, self.ns, at = [], [], 0
        for i in order:
            if i == 1:
                rows.append(torch.full_like(two.key_offsets[0], at))
                self.ns.append(0)
            else:
                rows.append(two.key_offsets[live.index(i)])
                self.ns.append(two.ns[live.index(i)])
                at += self.ns[-1]
        self.key_offsets = torch.stack(rows).contiguous()

    def ns_array(self):
        return (ctypes.c_int64 * len(self.ns))(*self.ns)


def test_batch_is_the_single_call_wherever_a_window_sits(ebos, lib):
    windows, voxels = batch_windows(), batch_voxels()
    assert [len(w) for w in windows] == [N, 0, 2 + len(range(1, N - 1)[::3])]
    plans = {0: M.plan_of(ebos, windows[0]), 2: M.plan_of(ebos, windows[2])}   # built once: a run's order is a build's own
    sh, K = c_shifts(plans[0], FML)
    pad, omit = 2, 1
    h, w = H + 2 * pad, W + 2 * pad
    refs = {i: M.ref_iwes(("batch", i), windows[i], voxels[i], FML, pad) for i in (0, 2)}
    g_images = G(np.random.RandomState(7).uniform(-1, 1, (B, K, h, w)), torch.float32)
    affine = G(np.random.RandomState(8).uniform(0.5, 2, (B, K, 2)), torch.float32)
    vox = G(np.stack(voxels), torch.float32)
    # each window alone, through the single entry points
    single = {}
    for i in (0, 2):
        d1 = torch.full((T5, 2, H, W), float("nan"), dtype=torch.float32, device=M.dev())
        p = plans[i]
        ok(lib.ebos_iwe_voxel_multiref_owner_bwd_f32(P(p.x), P(p.y), P(p.dt), P(p.bins), P(p.key_offsets), p.n, P(vox[i]), T5, H, W,
                                                     p.tile[0], p.tile[1], pad, pad, sh, K, P(g_images[i]), P(affine[i]), omit, P(d1), S()),
           lib)
        single[i] = d1
    for order in ((0, 1, 2), (2, 0, 1)):
        idx = list(order)
        st = Stack3(ebos, plans, idx)
        vbuf, v = guarded(values=vox[idx])
        obuf, iwes = guarded(shape=(B, K, h, w))
        iwes.zero_()
        ok(lib.ebos_iwe_voxel_multiref_tiled_batch_f32(P(st.x), P(st.y), P(st.dt), P(st.bins), P(st.key_offsets), st.ns_array(), B, P(v), T5,
                                                       H, W, st.tile[0], st.tile[1], 32, 2, pad, pad, sh, K, P(iwes), S()), lib)
        dbuf, d_voxel = guarded(shape=(B, T5, 2, H, W))
        ok(lib.ebos_iwe_voxel_multiref_owner_bwd_batch_f32(P(st.x), P(st.y), P(st.dt), P(st.bins), P(st.key_offsets), st.ns_array(), B, P(v),
                                                           T5, H, W, st.tile[0], st.tile[1], pad, pad, sh, K, P(g_images[idx].contiguous()),
                                                           P(affine[idx].contiguous()), omit, P(d_voxel), S()), lib)
        torch.cuda.synchronize()
        assert guards_untouched(vbuf) and guards_untouched(obuf) and guards_untouched(dbuf) and bool(torch.isfinite(d_voxel).all())
        for slot, i in enumerate(idx):
            if i == 1:                                              # the empty window: its images stay zero, its d_voxel is zeros
                assert int(torch.count_nonzero(iwes[slot])) == 0 and int(torch.count_nonzero(d_voxel[slot])) == 0
                continue
            for k in range(K):
                r = rel(iwes[slot, k], refs[i][k])
                print(f"order {order} window {i} reference {FML[k]!r}: IWE relative L2 {r:.3e}")
                assert r < 1e-4, (order, i, k)
            assert torch.equal(d_voxel[slot], single[i]), (order, i)   # the single call's bits, wherever the window sits
    assert not torch.equal(single[0], single[2])
