"""The general kernels behind ``event_based_bos_amd.ops`` (csrc/warp_kernels.hip, splat_kernels.hip, the templated kernels of
cost_kernels.hip, image_filters.hip) against the float64 CPU oracle, at the cases of tests/_ops_cases.py: past one launch wave of every
grid-stride loop, past kCostGrid rows and kCostBlock columns, K > 1 stacks, b > 1 batches, float32 and float64, forward and backward.
The ``ops`` functions are called directly, so the general kernels are what runs (never the fused idiom); a float32 case feeds the
oracle the same float32 values, upcast; gradients come from torch autograd of the oracle.

Bars (the project's own, header of tests/test_gpu_parity.py): warped events bit-exact; float64 images rel-L2 <= 1e-12, costs 1e-12,
gradients rel-L2 <= 1e-10; float32 images < 1e-5, costs < 1e-5, gradients rel-L2 < 1e-3.  Every test prints its errors on one
``OPS|`` line."""
import numpy as np
import pytest
import torch

import _ops_cases as C
from _ops_cases import O

pytestmark = pytest.mark.gpu

H, W = C.EVENT_IMAGE
IDS = {"ids": lambda c: c.id}
DT = {"ids": lambda d: np.dtype(d).name}
WARPS = (("middle", True), (0.25, False))


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def differing(got, want):
    """Elements that differ bit-wise in value (nan equals nan: 0 / 0 of a one-event window under normalize_t)."""
    return int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())


def report(op, tag, **errs):
    print("OPS|" + op + "|" + tag + "|" + "|".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in errs.items()))


def check(errs, dtype, what):
    for name, err in errs.items():
        assert C.passes(err, dtype, what), f"{name}: {err:.3e} against the {what} bar {C.bar(dtype, what):g} of {np.dtype(dtype).name}"


def mode_of(ebos, direction):
    from event_based_bos_amd.event_plan import parse_direction

    return parse_direction(direction)


# ---------------------------------------------------------------------------------------------------------------- time range
@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
def test_time_range_is_exact(ebos, dtype):
    """min / max per batch row, equal to numpy's: sorted and mixed-sign timestamps over three trips of the loop (several workgroups per
    row, one atomicMin / atomicMax each), a row of all-equal timestamps, n = 1."""
    windows = {"sorted": C.warp_events(C.EventCase(3, C.N_BIG, dtype)), "mixed": C.warp_events(C.EventCase(3, C.N_BIG, dtype, 0, True)),
               "n1": C.warp_events(C.EventCase(3, 1, dtype)), "n257": C.warp_events(C.EventCase(3, 257, dtype))}
    equal = C.warp_events(C.EventCase(3, 1031, dtype)).copy()
    equal[1, :, 2] = -0.25           # a negative constant: the initial (+inf, -inf) must lose on both sides
    equal[2, :, 2] = -equal[2, :, 2]  # an all-negative row
    windows["equal"] = equal
    for tag, ev in windows.items():
        got = N(ebos.ops.time_range(G(ev)))
        want = np.stack([ev[..., 2].min(axis=1), ev[..., 2].max(axis=1)], axis=1)
        report("time_range", f"{tag} {np.dtype(dtype).name}", mismatches=int((got != want).sum()))
        np.testing.assert_array_equal(got, want, err_msg=tag)
    assert (windows["mixed"][..., 2].min(axis=1) < 0).all() and (windows["mixed"][..., 2].max(axis=1) > 0).all()


# ---------------------------------------------------------------------------------------------------------------- warps, forward
WARP_CASES = tuple(c for c in C.BIG_EVENT_CASES if c.pad == 0) + C.MIXED_CASES + tuple(c for c in C.SMALL_EVENT_CASES if c.pad == 0 and c.n > 0)


@pytest.mark.parametrize("case", WARP_CASES, **IDS)
def test_warp_dense_is_bit_exact_and_counts_out_of_range(ebos, case):
    """Warped events bit for bit the oracle's torch branch in the same dtype; events whose source pixel lies outside the flow field keep
    their coordinates and are counted -- the counter holds the events planted in EVERY trip of the loop."""
    ev, flow = C.warp_events(case), C.flow_of(case)
    gev, gflow = G(ev), G(flow)
    for direction, norm in WARPS:
        want, bad = C.ref_warp_dense(ev, flow, direction, norm)
        oob = torch.zeros(1, dtype=torch.int32, device=gev.device)
        got = N(ebos.ops.warp_dense(gev, gflow, *mode_of(ebos, direction), norm, oob=oob))
        planted = case.b * len(C.oor_indices(case.n))
        report("warp_dense", f"{case.id} {direction} norm {int(norm)}", mismatches=differing(got, want), counted=int(oob.item()),
               planted=planted)
        np.testing.assert_array_equal(got, want)
        assert int(oob.item()) == planted == int(bad.sum())
        if case.n == C.N_BIG:
            per_trip = C.oor_per_trip(case.n)
            assert len(per_trip) >= 2 and min(per_trip) > 0 and case.b * sum(per_trip) == planted


@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
@pytest.mark.parametrize("n", (1, 257, C.N_BIG))
def test_warp_2dof_is_bit_exact(ebos, dtype, n):
    for mixed in (False, True) if n == C.N_BIG else (False,):
        ev = C.warp_events(C.EventCase(1, n, dtype, 0, mixed))[0]
        theta = np.array([2.5, -1.5], dtype=dtype)
        for direction, norm in WARPS:
            want = O.warp_2dof(torch.from_numpy(ev), torch.from_numpy(theta), direction, norm).numpy()
            got = N(ebos.ops.warp_2dof(G(ev), G(theta), *mode_of(ebos, direction), norm))
            report("warp_2dof", f"n {n} {np.dtype(dtype).name} mixed {int(mixed)} {direction} norm {int(norm)}", mismatches=differing(got, want))
            np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- warps, backward
@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
def test_warp_dense_backward(ebos, dtype):
    """d_flow for a random upstream gradient at b = 3: the blockIdx.y offsets of events, upstream and d_flow, both trips, out-of-range
    events skipped, and C.DUPLICATES events of every row on ONE source pixel (atomics on one address)."""
    case = C.EventCase(3, C.N_BIG, dtype)
    ev, flow, up = C.with_duplicates(C.warp_events(case)), C.flow_of(case), C.upstream_events(case)
    for direction, norm in WARPS:
        want = C.ref_warp_dense_backward(ev, flow, direction, norm, up)
        gflow = G(flow).requires_grad_(True)
        ebos.ops.warp_dense(G(ev), gflow, *mode_of(ebos, direction), norm).backward(G(up))
        got = N(gflow.grad)
        errs = {"d_flow": C.rel(got, want), "hot_pixel": C.rel(got[:, :, 17, 23], want[:, :, 17, 23]),
                "worst_row": max(C.rel(got[r], want[r]) for r in range(case.b))}
        report("warp_dense_bwd", f"{case.id} {direction} norm {int(norm)}", **errs)
        check(errs, dtype, "grad")


@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
def test_warp_2dof_backward(ebos, dtype):
    """d_theta at n_big: per-thread accumulators over three trips, a block sum and one atomic per workgroup; the upstream gradient has a
    non-zero mean, so the float32 sum does not cancel."""
    case = C.EventCase(1, C.N_BIG, dtype)
    ev, up = C.warp_events(case)[0], C.upstream_events(case)[0]
    theta = np.array([2.5, -1.5], dtype=dtype)
    for direction, norm in (("first", True), (0.25, False)):      # (dt of one sign over most of the window: the sums do not cancel)
        want = C.ref_warp_2dof_backward(ev, theta, direction, norm, up)
        gth = G(theta).requires_grad_(True)
        ebos.ops.warp_2dof(G(ev), gth, *mode_of(ebos, direction), norm).backward(G(up))
        errs = {"d_theta": C.rel(N(gth.grad), want), "worst_component": float(np.abs(N(gth.grad) / want - 1).max())}
        report("warp_2dof_bwd", f"{case.id} {direction} norm {int(norm)}", **errs)
        check(errs, dtype, "grad")


# ---------------------------------------------------------------------------------------------------------------- splat
def splat_all_modes(ebos, case):
    """(errors, allowed) of the three modes with per-event and scalar weights.  ``allowed`` is the project's image bar.  A float32
    quantity gets, next to its error, the error of the SAME sum in float32 on the CPU (``np.add.at`` in input order, ``cpu_*``): where
    that alone exceeds a tenth of the 1e-5 bar -- a constant weight that is no power of two, on the 1/64 px grid, makes the roundings
    of a float32 sum systematic: 1.65e-5 at 600 k events on 37 x 53 -- the kernel (atomics in arbitrary order) is allowed 10 x the
    CPU's float32 error, and never more than the north-star 1e-4."""
    from event_based_bos_amd import _hip

    ev, wt, pad = C.splat_events(case), C.weights_of(case), case.pad
    gev, gwt = G(ev), G(wt)
    size = C.padded(pad)
    f32 = case.dtype == np.float32
    errs, allowed = {}, {}

    def put(key, got, want, cpu_f32):
        errs[key] = C.rel(got, want)
        allowed[key] = C.bar(case.dtype, "image")
        if f32:
            errs["cpu_" + key] = C.rel(cpu_f32(), want)
            allowed[key] = min(max(allowed[key], 10.0 * errs["cpu_" + key]), 1e-4)

    for tag, weight, gweight in (("w", wt, gwt), ("s", 0.7, 0.7)):
        w32 = wt if tag == "w" else np.full(wt.shape, 0.7, dtype=np.float32)
        got = N(ebos.ops.splat(gev, size, (pad, pad), gweight, _hip.SPLAT_BILINEAR))
        assert got.shape == (case.b,) + size and got.dtype == case.dtype
        want = C.ref_splat(ev, pad, weight)
        put("bilinear_" + tag, got, want, lambda: C.ref_splat_f32_in_order(ev, pad, w32))
        errs["bilinear_worst_row_" + tag] = max(C.rel(got[r], want[r]) for r in range(case.b))
        allowed["bilinear_worst_row_" + tag] = allowed["bilinear_" + tag]
        got = N(ebos.ops.splat(gev, size, (pad, pad), gweight, _hip.SPLAT_POLARITY))
        assert got.shape == (case.b, 2) + size
        pos = ev[..., 3] > 0        # (a zero weight adds 0.0f: the float32 sum of a plane in input order)
        put("polarity_" + tag, got, C.ref_polarity(ev, pad, weight),
            lambda: np.stack([C.ref_splat_f32_in_order(ev, pad, w32 * m) for m in (pos, ~pos)], axis=1))
    got = N(ebos.ops.splat(gev, size, (pad, pad), 1.0, _hip.SPLAT_COUNT))
    errs["count_mismatches"] = int((got != C.ref_count(ev, pad)).sum())
    return errs, allowed


def check_splat(errs, allowed, dtype):
    assert errs["count_mismatches"] == 0
    for key, bar in allowed.items():
        assert errs[key] <= bar if np.dtype(dtype) == np.float64 else errs[key] < bar, f"{key}: {errs[key]:.3e} against {bar:.3e}"


@pytest.mark.parametrize("case", C.BIG_EVENT_CASES, **IDS)
def test_splat_forward(ebos, case):
    """bilinear vote, count and polarity images of n_big events, b in {1, 3}, both pads: every eighth event has taps outside the padded
    image, each of the four masked on its own.  Counts are exact."""
    errs, allowed = splat_all_modes(ebos, case)
    report("splat", case.id, **errs)
    check_splat(errs, allowed, case.dtype)


@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
def test_splat_forward_small_counts(ebos, dtype):
    """n in {0, 1, 255, 256, 257} at b = 3: no event, one lane, one wave short of / exactly / one past a workgroup."""
    for case in C.SMALL_EVENT_CASES:
        if case.dtype != dtype:
            continue
        errs, allowed = splat_all_modes(ebos, case)
        report("splat", case.id, **errs)
        check_splat(errs, allowed, dtype)


@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
@pytest.mark.parametrize("pad", (0, 2))
def test_splat_backward(ebos, dtype, pad):
    """d_events and d_weight of the bilinear vote at b = 3, n_big, for a random upstream image per batch row."""
    case = C.EventCase(3, C.N_BIG, dtype, pad)
    ev, wt, up = C.splat_events(case), C.weights_of(case), C.upstream_image(case)
    want_e, want_w = C.ref_splat_backward(ev, pad, wt, up)
    gev, gwt = G(ev).requires_grad_(True), G(wt).requires_grad_(True)
    ebos.ops.splat(gev, C.padded(pad), (pad, pad), gwt).backward(G(up))
    got_e, got_w = N(gev.grad), N(gwt.grad)
    m = C.trips(case.n, *C.limits()["splat_bwd_kernel"])[2]
    errs = {"d_events": C.rel(got_e, want_e), "d_weight": C.rel(got_w, want_w), "d_events_last_trip": C.rel(got_e[:, m:], want_e[:, m:]),
            "d_weight_rows": max(C.rel(got_w[r], want_w[r]) for r in range(case.b))}
    report("splat_bwd", case.id, **errs)
    check(errs, dtype, "grad")
    assert (got_e[..., 2:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- costs
def cost_errors(ebos, name, x, omit, upstream):
    fn = {"var": ebos.ops.image_variance, "gm": ebos.ops.gradient_magnitude}[name]
    gx = G(x).requires_grad_(True)
    vals = fn(gx, omit)
    assert vals.shape == (x.shape[0],) and vals.dtype == gx.dtype
    vals.backward(G(upstream))
    want_v, want_g = C.ref_cost(name, x, omit, upstream)
    got_g = N(gx.grad)
    return ({"value": float(np.abs(N(vals).astype(np.float64) / want_v - 1).max())},
            {"grad": C.rel(got_g, want_g), "grad_worst_image": max(C.rel(got_g[k], want_g[k]) for k in range(x.shape[0]))})


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("omit", (False, True))
@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
@pytest.mark.parametrize("name", ("var", "gm"))
def test_costs_beyond_the_reduction_grid(ebos, name, dtype, omit, K):
    """Value and d / d image on 243 x 259 stacks: more region rows than kCostGrid and more region columns than kCostBlock, with and
    without the boundary; the K = 3 upstream differs per image ([K][grid][2] partials, blockIdx.y offsets of the gradient kernels)."""
    x = C.images(K, C.COST_IMAGE, dtype)
    cost, grad = cost_errors(ebos, name, x, omit, C.upstream_costs(K, dtype))
    report(name, "%dx%d K %d omit %d %s" % (C.COST_IMAGE + (K, int(omit), np.dtype(dtype).name)), **cost, **grad)
    check(cost, dtype, "cost")
    check(grad, dtype, "grad")


@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
@pytest.mark.parametrize("name", ("var", "gm"))
def test_costs_beyond_one_wave_of_pixels(ebos, name, dtype):
    """601 x 1801: the element-wise gradient kernels take a second, ragged trip under the largest cap."""
    x = C.images(1, C.PIXEL_IMAGE, dtype)
    h, w = C.PIXEL_IMAGE
    for omit in (False, True):
        cost, grad = cost_errors(ebos, name, x, omit, C.upstream_costs(1, dtype))
        report(name, "%dx%d K 1 omit %d %s" % (h, w, int(omit), np.dtype(dtype).name), **cost, **grad)
        check(cost, dtype, "cost")
        check(grad, dtype, "grad")


@pytest.mark.parametrize("omit", (False, True))
@pytest.mark.parametrize("shape", C.DEGENERATE, ids=lambda s: "%dx%d" % s)
def test_costs_on_degenerate_regions(ebos, shape, omit):
    """Regions of 0 and 1 pixels (and the smallest regular ones): value and gradient equal torch's, nan where torch says nan."""
    for dtype in C.DTYPES:
        for name in ("var", "gm"):
            x = C.images(2, shape, dtype)
            up = C.upstream_costs(2, dtype)
            fn = {"var": ebos.ops.image_variance, "gm": ebos.ops.gradient_magnitude}[name]
            gx = G(x).requires_grad_(True)
            vals = fn(gx, omit)
            vals.backward(G(up))
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")            # (torch.var of fewer than two values warns about the degrees of freedom)
                want_v, want_g = C.ref_cost(name, x, omit, up)
            got_v, got_g = N(vals).astype(np.float64), N(gx.grad).astype(np.float64)
            report(name, "%dx%d omit %d %s" % (shape + (int(omit), np.dtype(dtype).name)), value=str(got_v.tolist()), torch=str(want_v.tolist()),
                   nan_in_grad=int(np.isnan(got_g).sum()), nan_in_torch_grad=int(np.isnan(want_g).sum()))
            # (absolute floor: the rounding of the float64 yardstick itself -- torch's convolution leaves 2e-31 where the Sobel of
            # one replicated pixel is exactly zero; both costs are bounded by max x^2)
            floor = np.finfo(np.float64).eps * float(np.square(x.astype(np.float64)).max())
            np.testing.assert_allclose(got_v, want_v, rtol=C.bar(dtype, "cost"), atol=floor, equal_nan=True)
            assert np.array_equal(np.isnan(got_g), np.isnan(want_g))
            scale = np.abs(np.nan_to_num(want_g)).max()
            floor = np.finfo(np.float64).eps * float(np.abs(x).max()) * float(np.abs(up).max())     # (the same rounding, differentiated)
            np.testing.assert_allclose(got_g, want_g, rtol=0, atol=C.bar(dtype, "grad") * scale + floor, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- blur passes
@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
@pytest.mark.parametrize("axis,boundary,radius", C.GAUSS_CASES)
def test_gauss1d_beyond_one_wave_of_pixels(ebos, dtype, axis, boundary, radius):
    """One blur pass and its adjoint on 601 x 1801 against the dense operator of the library the reference calls (scipy correlate1d
    'reflect' / torch reflect pad + conv1d, as test_blur_pass_adjoint), with taps that are not symmetric."""
    x = C.images(1, C.PIXEL_IMAGE, dtype)[0]
    gy = C.images(1, C.PIXEL_IMAGE, dtype, seed=32)[0] - dtype(3.0)
    taps = C.gauss_taps(radius)
    A = C.gauss_operator(x.shape[axis], taps, boundary)
    gx = G(x).requires_grad_(True)
    y = ebos.ops.gauss1d(gx, axis, torch.from_numpy(taps), boundary)
    y.backward(G(gy))
    fwd = {"forward": C.rel(N(y), C.apply_along(A, x, axis))}
    adj = {"adjoint": C.rel(N(gx.grad), C.apply_along(A.T, gy, axis))}
    report("gauss1d", f"axis {axis} boundary {boundary} radius {radius} {np.dtype(dtype).name}", **fwd, **adj)
    check(fwd, dtype, "image")
    check(adj, dtype, "grad")


# ---------------------------------------------------------------------------------------------------------------- the chain
def direct_chain(ebos, ev, flow, pad, upstream):
    from event_based_bos_amd import _hip

    gflow = G(flow).requires_grad_(True)
    warped = ebos.ops.warp_dense(G(ev), gflow, *mode_of(ebos, C.CHAIN_DIRECTION), True)
    iwe = ebos.ops.splat(warped, C.padded(pad), (pad, pad), 1.0, _hip.SPLAT_BILINEAR)
    var = ebos.ops.image_variance(iwe, C.CHAIN_OMIT)
    var.backward(G(upstream))
    return warped.detach(), iwe.detach(), var.detach(), gflow.grad


@pytest.mark.parametrize("dtype", C.DTYPES, **DT)
def test_chain_warp_splat_variance_backward(ebos, dtype):
    """warp_dense -> splat -> image_variance -> backward at b = 3, n_big, pad 2, one upstream factor per batch row; the events keep
    5e-4 px from the kinks of the vote (tests/_kinks.py), where float32 and float64 may take different one-sided derivatives."""
    pad = 2
    ev, flow = C.chain_inputs(dtype)
    up = C.upstream_costs(3, dtype)
    warped, iwe, var, d_flow = direct_chain(ebos, ev, flow, pad, up)
    want_warped, want_iwe, want_var, want_d = C.ref_chain(ev, flow, pad, up)
    same = O.warp_dense_torch(torch.from_numpy(ev), torch.from_numpy(flow), C.CHAIN_DIRECTION, True).numpy()
    np.testing.assert_array_equal(N(warped), same)      # bit-exact in the same dtype
    img = {"iwe": C.rel(N(iwe), want_iwe)}
    cost = {"variance": float(np.abs(N(var).astype(np.float64) / want_var - 1).max())}
    grad = {"d_flow": C.rel(N(d_flow), want_d), "d_flow_worst_row": max(C.rel(N(d_flow)[r], want_d[r]) for r in range(3))}
    report("chain", f"b3-n{ev.shape[1]}-{np.dtype(dtype).name}-pad{pad}", warped_vs_f64=C.rel(N(warped), want_warped), **img, **cost, **grad)
    check(img, dtype, "image")
    check(cost, dtype, "cost")
    check(grad, dtype, "grad")


def test_public_surface_batched_float32(ebos):
    """The same chain through Warp.warp_event + EventImageConverter.bilinear_vote_tensor with batched float32 GPU tensors (never
    lazy-eligible: the general kernels run): warped events bit for bit the direct ``ops`` call's, the image within the image bar of
    it and of the oracle, the flow gradient within the gradient bar."""
    dtype, pad = np.float32, 2
    ev, flow = C.chain_inputs(dtype)
    up = C.upstream_costs(3, dtype)
    warped, iwe, var, d_flow = direct_chain(ebos, ev, flow, pad, up)
    gflow = G(flow).requires_grad_(True)
    warper, imager = ebos.Warp(C.EVENT_IMAGE, normalize_t=True), ebos.EventImageConverter(C.EVENT_IMAGE, outer_padding=pad)
    w2, _ = warper.warp_event(G(ev), gflow, "dense-flow", C.CHAIN_DIRECTION)
    assert type(w2) is torch.Tensor and w2.is_cuda and w2.dtype == torch.float32
    i2 = imager.bilinear_vote_tensor(w2)
    assert type(i2) is torch.Tensor and tuple(i2.shape) == (3,) + C.padded(pad)
    ebos.ops.image_variance(i2, C.CHAIN_OMIT).backward(G(up))
    warper.check_out_of_range()
    _, want_iwe, _, want_d = C.ref_chain(ev, flow, pad, up)
    np.testing.assert_array_equal(N(w2), N(warped))
    img = {"iwe_vs_ops": C.rel(N(i2), N(iwe)), "iwe_vs_oracle": C.rel(N(i2), want_iwe)}
    grad = {"d_flow_vs_ops": C.rel(N(gflow.grad), N(d_flow)), "d_flow_vs_oracle": C.rel(N(gflow.grad), want_d)}
    report("surface", f"b3-n{ev.shape[1]}-float32-pad{pad}", **img, **grad)
    check(img, dtype, "image")
    check(grad, dtype, "grad")
