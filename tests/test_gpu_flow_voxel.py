"""GPU checks of the time-aware flow kernels (csrc/flow_voxel.hip) against tests/_flow_voxel_ref.py, the restatement that
tests/test_flow_voxel.py pins to the reference's own arrays.

The advection kernels evaluate the reference's expressions with every operation rounded on its own, so steps, chains and copies are
compared with ``np.array_equal`` (NaN in the same places), float64 and float32.  The bilinear votes are the reference's addends added
by atomics in a free order: per cell |gpu - sequential| <= 2 k u sum|w| (k votes, u = 2^-53 or 2^-24), and a cell
nothing votes into is exactly 0.

Shapes: the 32 x 32 tile of the chain kernel gives (32, 32) = one tile, (33, 33) = a tile plus one, (70, 130) = 3 x 5 tiles with a
ragged edge; (1, 1), (1, 7), (7, 1), (2, 3) are smaller than any halo.  The chain is one launch up to ``halo_cap()`` = 8 steps per
direction: bins 8 and 9 ('first': 7 and 8 steps) are its last two sizes, 10 ('first') and 19 ('middle': 9 each way) take a launch per
step.  Nothing depends on a larger size: the indices are 64-bit throughout.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _flow_voxel_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (32, 32), (33, 33), (70, 130)]
BINS = (1, 2, 3, 8, 9, 10, 19)
STEPS = [(0.2, 1, 1), (-0.25, 2, 4)]
STEP_FN = {"upwind": R.upwind_step, "burgers": R.burgers_step}
CLAMP = 1.5
_cache = {}


def flows(shape, B=3):
    """B flows in [-3, 3] with both signs, exact zeros and one NaN pixel (in flow 0, component 1)."""
    key = ("flows", shape, B)
    if key not in _cache:
        rs = np.random.RandomState(6000 + 131 * shape[0] + shape[1])
        f = rs.uniform(-3.0, 3.0, (B, 2) + shape)
        f[rs.uniform(size=f.shape) < 0.15] = 0.0
        f[0, 1, shape[0] // 2, shape[1] // 3] = np.nan
        f.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def reference(shape, dtype, scheme, T, loc, wrap):
    """The restated voxel of the three flows, unclamped: numpy for float64 without the wrap, CPU torch otherwise."""
    key = ("ref", shape, dtype, scheme, T, loc, wrap and scheme == "burgers" and R.t0_index(loc, T) == T - 1)
    if key not in _cache:
        f = flows(shape).astype(dtype)
        if wrap or dtype == np.float32:
            _cache[key] = R.construct(torch.from_numpy(f), T, scheme, loc, None, torch_wrap=wrap).numpy()
        else:
            _cache[key] = R.construct(f, T, scheme, loc, None)
    return _cache[key]


def equal(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_constructors_match_the_restatement_bit_for_bit(shape, dtype):
    from event_based_bos_amd.utils import construct_dense_flow_voxel_numpy, construct_dense_flow_voxel_torch

    f = flows(shape).astype(dtype)
    dev = torch.from_numpy(f).cuda()
    multi = shape == (70, 130)
    for scheme in ("upwind", "burgers", "same"):
        for T in BINS:
            for loc in ("first", "middle"):
                want = reference(shape, dtype, scheme, T, loc, True)
                # B = 3 clamped and B = 1 unclamped everywhere; the other two pairings on the multi-tile shape
                for B, clamp in ((3, CLAMP), (1, None)) + (((3, None), (1, CLAMP)) if multi else ()):
                    w = want[:B] if clamp is None else np.clip(want[:B], -clamp, clamp)
                    got = construct_dense_flow_voxel_torch(dev[:B], T, scheme, loc, clamp)
                    assert got.is_cuda and equal(got, w), (scheme, T, loc, B, clamp)
                assert equal(construct_dense_flow_voxel_torch(dev[1], T, scheme, loc), want[1]), (scheme, T, loc)   # 3-D in, 4-D out
                if dtype == np.float64:
                    wn = reference(shape, dtype, scheme, T, loc, False)
                    got = construct_dense_flow_voxel_numpy(f, T, scheme, loc, CLAMP)
                    assert isinstance(got, np.ndarray) and equal(got, np.clip(wn, -CLAMP, CLAMP)), (scheme, T, loc)
    if dtype == np.float32:     # the numpy constructor is float64 whatever comes in
        got = construct_dense_flow_voxel_numpy(f[0], 3, "upwind", "middle")
        assert equal(got, R.construct(f[:1].astype(np.float64), 3, "upwind", "middle")[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_single_steps_match_the_restatement_bit_for_bit(shape, dtype):
    """Also the reference's squeeze: every size-1 axis of the result goes."""
    from event_based_bos_amd import utils

    f = flows(shape).astype(dtype)
    for scheme, stem in (("upwind", "upwind_flow_to_voxel_"), ("burgers", "inviscid_burger_flow_to_voxel_")):
        for dt, dx, dy in STEPS:
            want = STEP_FN[scheme](torch.from_numpy(f), dt, dx, dy).numpy()
            got = getattr(utils, stem + "torch")(torch.from_numpy(f).cuda(), dt, dx, dy)
            assert got.is_cuda and equal(got, np.squeeze(want)), (scheme, dt)
            got = getattr(utils, stem + "torch")(torch.from_numpy(f[0]), dt, dx, dy)         # 3-D, from the host
            assert not got.is_cuda and equal(got, np.squeeze(want[0])), (scheme, dt)
            if dtype == np.float64:
                got = getattr(utils, stem + "numpy")(f, dt, dx, dy)
                assert isinstance(got, np.ndarray) and equal(got, np.squeeze(STEP_FN[scheme](f, dt, dx, dy))), (scheme, dt)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fused_route_and_per_step_route_store_the_same_bits(dtype):
    from event_based_bos_amd import _hip, flow_voxel

    dev = torch.from_numpy(flows((70, 130))).cuda().to(dtype)
    assert flow_voxel.halo_cap() == 8
    try:
        for scheme in ("upwind", "burgers"):
            for T, loc in ((8, "first"), (9, "first"), (17, "middle"), (2, "middle"), (1, "first")):
                for clamp, wrap in ((None, False), (CLAMP, True)):
                    out = {}
                    for route in (_hip.FLOW_ROUTE_FUSED, _hip.FLOW_ROUTE_STEPS):
                        flow_voxel._FORCE_ROUTE = route
                        out[route] = flow_voxel.flow_voxel_batch(dev, T, scheme, loc, clamp, torch_burgers_wrap=wrap)
                    a, b = (o.cpu().numpy() for o in out.values())
                    assert np.array_equal(a, b, equal_nan=True), (scheme, T, loc, clamp, wrap)
        flow_voxel._FORCE_ROUTE = _hip.FLOW_ROUTE_FUSED
        with pytest.raises(RuntimeError, match="do not fit a halo"):
            flow_voxel.flow_voxel_batch(dev, 10, "upwind", "first")
    finally:
        flow_voxel._FORCE_ROUTE = None


def test_batch_equals_the_single_calls():
    from event_based_bos_amd import flow_voxel_batch

    for dtype in (torch.float64, torch.float32):
        dev = torch.from_numpy(flows((33, 33))).cuda().to(dtype)
        for scheme in ("upwind", "burgers", "same"):    # (bilinear in a batch: test_bilinear_votes_within_the_summation_bound)
            for T, loc in ((5, "middle"), (10, "first")):
                batch = flow_voxel_batch(dev, T, scheme, loc, CLAMP)
                assert batch.shape == (3, T, 2, 33, 33) and batch.dtype == dtype
                singles = torch.cat([flow_voxel_batch(dev[b:b + 1], T, scheme, loc, CLAMP) for b in range(3)])
                assert np.array_equal(batch.cpu().numpy(), singles.cpu().numpy(), equal_nan=True), (scheme, T, loc)
        out = torch.empty((3, 5, 2, 33, 33), dtype=dtype, device="cuda")
        assert flow_voxel_batch(dev, 5, "upwind", "middle", out=out) is out
        assert np.array_equal(out.cpu().numpy(), flow_voxel_batch(dev, 5, "upwind", "middle").cpu().numpy(), equal_nan=True)
        with pytest.raises(ValueError):
            flow_voxel_batch(dev, 5, "upwind", "middle", out=out[:, :4])
    with pytest.raises(ValueError):
        flow_voxel_batch(torch.zeros(2, 2, 4, 4), 3)                 # not on the GPU
    buf = torch.zeros(3 * 2 * 4 * 4, dtype=torch.float64, device="cuda")
    for scheme in ("upwind", "same", "bilinear"):                    # out must not share memory with the flows
        with pytest.raises(ValueError, match="overlap"):
            flow_voxel_batch(buf[64:].view(1, 2, 4, 4), 3, scheme, "first", out=buf.view(1, 3, 2, 4, 4))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_truncate_matches_the_restatement_bit_for_bit(dtype):
    from event_based_bos_amd.utils import truncate_voxel_flow_numpy

    for shape, T in (((70, 130), 7), ((2, 3), 1), ((1, 1), 4)):
        rs = np.random.RandomState(77)
        voxel = rs.uniform(-2.0, 2.0, (T, 2) + shape)
        voxel[np.broadcast_to(rs.uniform(size=(T, 1) + shape) < 0.3, voxel.shape)] = 0.0      # bins without flow at a pixel
        voxel[:, :, 0, 0] = 0.0                                                               # a pixel no bin has flow at
        voxel[0, 0, -1, -1] = 1e-200 if dtype == np.float64 else 1e-30                         # u u underflows: masked unless v counts
        voxel = voxel.astype(dtype)
        got = truncate_voxel_flow_numpy(voxel)
        assert equal(got, R.truncate_mean(voxel)) and got.dtype == np.float64


def converging(shape, dtype):
    """A flow towards the middle of the image plus noise: with dt = 1 many votes land in few cells; with dt = -1 most leave the image."""
    H, W = shape
    rs = np.random.RandomState(91)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = np.stack([(H / 2 - ii) * 0.9, (W / 2 - jj) * 0.9]) + rs.uniform(-1.5, 1.5, (2, H, W))
    return f.astype(dtype)


def within_bound(got, ref, u):
    want, k, sabs = ref
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype
    err, bound = np.abs(got.astype(np.float64) - want.astype(np.float64)), 2.0 * k * u * sabs
    print(f"max |gpu - ref| {err.max():.3e}, worst share of the bound {(err / np.where(bound > 0, bound, 1.0)).max():.3f}, "
          f"{int((k == 0).sum())} cells without a vote, up to {int(k.max())} votes in a cell")
    assert (got[k == 0] == 0).all()
    assert (err <= bound).all(), (float(err.max()), int((err > bound).sum()))


@pytest.mark.parametrize("dtype,u", [(np.float64, 2.0 ** -53), (np.float32, 2.0 ** -24)])
def test_bilinear_votes_within_the_summation_bound(dtype, u):
    from event_based_bos_amd.utils import (construct_dense_flow_voxel_numpy, construct_dense_flow_voxel_torch,
                                           propagate_flow_to_voxel_numpy, propagate_flow_to_voxel_torch)

    for shape in ((70, 130), (7, 1), (1, 1)):
        f = converging(shape, dtype)
        for dt in (1.0, -1.0, 0.37, 0.0):
            ref = tuple(np.squeeze(a) for a in R.propagate_bilinear(f, dt))
            assert shape != (70, 130) or dt != 1.0 or ref[1].max() >= 8
            got = propagate_flow_to_voxel_torch(torch.from_numpy(f).cuda(), dt, "bilinear")
            assert got.is_cuda
            within_bound(got, ref, u)
            if dtype == np.float64:
                within_bound(propagate_flow_to_voxel_numpy(f, dt, "bilinear"), ref, u)
    batch = np.stack([converging((33, 40), dtype), -converging((33, 40), dtype)])
    for T, loc in ((3, "first"), (4, "middle")):
        voxel, k, sabs = R.construct_bilinear(batch, T, loc)
        within_bound(construct_dense_flow_voxel_torch(torch.from_numpy(batch).cuda(), T, "bilinear", loc), (voxel, k, sabs), u)
        # clipping moves no two values further apart
        within_bound(construct_dense_flow_voxel_torch(torch.from_numpy(batch).cuda(), T, "bilinear", loc, 2),
                     (np.clip(voxel, -2, 2), k, sabs), u)
        if dtype == np.float64:
            within_bound(construct_dense_flow_voxel_numpy(batch[0], T, "bilinear", loc), (voxel[0], k[0], sabs[0]), u)


def test_containers_dtypes_and_the_burgers_kink():
    from event_based_bos_amd import utils

    f = np.array(flows((7, 1)))
    f[np.isnan(f)] = 0.5
    for dtype in (torch.float32, torch.float64):
        dev = torch.from_numpy(f).cuda().to(dtype)
        for scheme in ("upwind", "burgers", "same", "bilinear"):
            got = utils.construct_dense_flow_voxel_torch(dev, 4, scheme)
            assert got.device == dev.device and got.dtype == dtype and got.shape == (3, 4, 2, 7, 1)     # the rank is kept for W = 1
            host = utils.construct_dense_flow_voxel_torch(dev.cpu(), 4, scheme)
            assert not host.is_cuda and host.dtype == dtype
            if scheme != "bilinear":
                assert torch.equal(host, got.cpu())
    got = utils.construct_dense_flow_voxel_numpy(f.astype(np.float32), 4)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (3, 4, 2, 7, 1)
    assert utils.construct_dense_flow_voxel_numpy(f.astype(np.int64)[0], 2, "same").dtype == np.float64
    # time_bin == 1, Burgers: the torch constructor's only bin is one backward step with dt = 1, the numpy constructor's is the input
    t = utils.construct_dense_flow_voxel_torch(torch.from_numpy(f).cuda(), 1, "burgers")
    assert equal(t[:, 0], R.burgers_step(f, -1.0)) and not np.array_equal(t[:, 0].cpu().numpy(), f)
    assert equal(utils.construct_dense_flow_voxel_numpy(f, 1, "burgers")[:, 0], f)
    assert equal(utils.construct_dense_flow_voxel_torch(torch.from_numpy(f).cuda(), 1, "upwind")[:, 0], f)
    # 'same' of the stand-alone function is a copy in the caller's container
    same = utils.propagate_flow_to_voxel_torch(torch.from_numpy(f[0]).cuda(), 0.3, "same")
    assert same.is_cuda and same.shape == (2, 7) and equal(same, np.squeeze(f[0]))
