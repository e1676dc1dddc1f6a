"""CPU checks of the time-aware flow (event_based_bos_amd/flow_voxel.py): tests/_flow_voxel_ref.py, the restatement the GPU tests
compare with, is pinned to arrays the reference itself produced (tests/golden/golden_flow_voxel.npz, written by
make_golden_flow_voxel.py) and to closed forms; the product's argument errors and its surface need no GPU."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _flow_voxel_ref as R  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "golden_flow_voxel.npz"))
STEPS = [(0.2, 1, 1), (-0.25, 2, 4)]      # as in make_golden_flow_voxel.py
DTS = [0.4, -0.7]
BINS = (1, 2, 3, 5)
STEP_FN = {"upwind": R.upwind_step, "burgers": R.burgers_step}
NAMES = ("construct_dense_flow_voxel_numpy", "construct_dense_flow_voxel_torch", "propagate_flow_to_voxel_numpy",
         "propagate_flow_to_voxel_torch", "upwind_flow_to_voxel_numpy", "upwind_flow_to_voxel_torch",
         "inviscid_burger_flow_to_voxel_numpy", "inviscid_burger_flow_to_voxel_torch", "truncate_voxel_flow_numpy",
         "convert_flow_per_bin_to_flow_per_sec")


def variants():
    f = G["flows"]
    return {"np": f, "t64": torch.from_numpy(f), "t32": torch.from_numpy(f.astype(np.float32))}


def arr(a):
    return a.numpy() if isinstance(a, torch.Tensor) else a


def same(got, want):
    got = arr(got)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("scheme", ["upwind", "burgers"])
def test_restated_steps_are_the_references(scheme):
    for k, (dt, dx, dy) in enumerate(STEPS):
        for v, f in variants().items():
            assert same(STEP_FN[scheme](f, dt, dx, dy), G[f"step_{scheme}_{k}_{v}"]), (k, v)


@pytest.mark.parametrize("scheme", ["upwind", "burgers"])
def test_restated_constructors_are_the_references(scheme):
    """Including the torch Burgers constructor's extra backward step, which shows for T = 1 and for T = 2 with t0 in the middle."""
    for v, f in variants().items():
        for T in BINS:
            for loc in ("first", "middle"):
                got = R.construct(f, T, scheme, loc, None, torch_wrap=v != "np")
                assert same(got, G[f"vox_{scheme}_{T}_{loc}_{v}"]), (T, loc, v)
        assert same(R.construct(f, 5, scheme, "middle", 1, torch_wrap=v != "np"), G[f"voxc_{scheme}_5_middle_{v}"]), v
    if scheme == "burgers":
        f = variants()["t64"]
        assert not np.array_equal(G["vox_burgers_1_first_t64"], G["vox_burgers_1_first_np"])
        assert not np.array_equal(G["vox_burgers_2_middle_t64"], G["vox_burgers_2_middle_np"])
        assert np.array_equal(G["vox_burgers_1_first_t64"][:, 0], arr(R.burgers_step(f, -1.0)))
        assert np.array_equal(G["vox_burgers_3_middle_t64"], G["vox_burgers_3_middle_np"])


def test_restated_bilinear_votes_and_truncate_are_the_references():
    """numpy's add.at and torch's CPU scatter_add_ both add the votes one after the other in the order of the list."""
    for k, dt in enumerate(DTS):
        for v, f in variants().items():
            out, votes, sabs = R.propagate_bilinear(arr(f)[0], dt)
            assert same(out, G[f"bil_{k}_{v}"]), (k, v)
            assert votes.max() >= 2 and ((votes == 0) == (sabs == 0)).all()
    assert same(R.truncate_mean(G["trunc_in"]), G["trunc"])


@pytest.mark.parametrize("scheme", ["upwind", "burgers"])
def test_a_uniform_flow_is_a_fixed_point(scheme):
    for u, v in ((1.5, -0.75), (-2.0, 3.0), (0.0, 1.0)):
        f = np.empty((2, 2, 5, 6))
        f[:, 0], f[:, 1] = u, v
        for T, loc in ((1, "first"), (4, "first"), (5, "middle")):
            voxel = R.construct(f, T, scheme, loc)
            assert voxel.shape == (2, T, 2, 5, 6) and all(np.array_equal(voxel[:, t], f) for t in range(T))
            assert np.array_equal(arr(R.construct(torch.from_numpy(f), T, scheme, loc, torch_wrap=True)), voxel)


def test_upwind_of_a_flow_linear_in_x_is_the_closed_form():
    """u = a i >= 0, v = 0: the backward difference is a everywhere below row 0, so one step gives a i - dt (a i) a; a, dt powers of two."""
    a, dt, H, W = 0.5, 0.25, 6, 4
    f = np.zeros((1, 2, H, W))
    f[0, 0] = a * np.arange(H)[:, None]
    got = R.upwind_step(f, dt)
    want = np.zeros_like(f)
    want[0, 0] = (a * np.arange(H) - dt * (a * np.arange(H) * a))[:, None]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("scheme", ["upwind", "burgers"])
def test_zero_dt_is_the_identity_and_backward_is_forward_of_the_negated_flow(scheme):
    f = G["flows"]
    assert STEP_FN[scheme](f, 0) is f
    assert np.array_equal(STEP_FN[scheme](f, -0.3, 2, 4), -STEP_FN[scheme](-f, 0.3, 2, 4))
    from event_based_bos_amd import utils

    for x in (f, torch.from_numpy(f)):     # returned before anything touches the GPU
        kind = "numpy" if isinstance(x, np.ndarray) else "torch"
        name = {"upwind": "upwind_flow_to_voxel_", "burgers": "inviscid_burger_flow_to_voxel_"}[scheme] + kind
        assert getattr(utils, name)(x, 0) is x and getattr(utils, name)(x, 0.0, 2, 3) is x


def test_truncate_of_equal_bins():
    """n equal bins b: n b / (n + 1e-6); against b (n / (n + 1e-6)) that is two roundings on either side."""
    b = G["flows"][0]
    b = np.where(b == 0.0, 1.0, b)
    for n in (1, 4, 7):
        got = R.truncate_mean(np.stack([b] * n))
        assert np.allclose(got, b * (n / (n + 1e-6)), rtol=2.0 ** -50, atol=0.0)
    zero = np.zeros((3, 2, 4, 5))
    assert np.array_equal(R.truncate_mean(zero), zero[0])      # 0 / 1e-6


def test_argument_errors_come_before_the_gpu():
    from event_based_bos_amd import utils

    f = G["flows"]
    for ctor, x in ((utils.construct_dense_flow_voxel_numpy, f), (utils.construct_dense_flow_voxel_torch, torch.from_numpy(f))):
        with pytest.raises(NotImplementedError, match="t0_location"):
            ctor(x, 3, "upwind", "last")
        with pytest.raises(NotImplementedError, match="unknown scheme"):
            ctor(x, 3, "zero", "first")
        with pytest.raises(NotImplementedError, match="torch_scatter"):
            ctor(x, 3, "max")
        for scheme in ("nearest", "linear", "cubic"):
            with pytest.raises(NotImplementedError, match="griddata"):
                ctor(x, 3, scheme)
        with pytest.raises(ValueError):
            ctor(x, 0)
    with pytest.raises(NotImplementedError, match="t0_location"):
        utils.flow_voxel_batch(torch.from_numpy(f), 3, "upwind", "last")
    for prop, x in ((utils.propagate_flow_to_voxel_numpy, f[0]), (utils.propagate_flow_to_voxel_torch, torch.from_numpy(f[0]))):
        with pytest.raises(NotImplementedError, match="griddata"):
            prop(x, 0.5)                              # the reference's default method, "nearest"
        with pytest.raises(NotImplementedError, match="torch_scatter"):
            prop(x, 0.5, "max")
        with pytest.raises(NotImplementedError, match="unknown method"):
            prop(x, 0.5, "spline")
        same_copy = prop(x, 0.5, "same")               # plain copy, no GPU
        assert same_copy is not x and np.array_equal(arr(same_copy), f[0])
    with pytest.raises(NotImplementedError, match="4-D"):
        utils.truncate_voxel_flow_numpy(f[0])
    with pytest.raises(NotImplementedError, match="median"):
        utils.truncate_voxel_flow_numpy(f, "median")
    ts = torch.tensor([[2.0], [4.0]])
    assert torch.equal(utils.convert_flow_per_bin_to_flow_per_sec(torch.from_numpy(f), ts, 5), torch.from_numpy(f) / ts[..., None, None])


def test_surface_has_the_references_names_and_signatures():
    from event_based_bos_amd import _hip, flow_voxel, utils

    want = json.load(open(os.path.join(HERE, "golden", "flow_voxel_signatures.json")))
    assert sorted(want) == sorted(NAMES)
    for name in NAMES:
        fn = getattr(utils, name)
        assert fn is getattr(flow_voxel, name)
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(fn).parameters.values()]
        assert got == want[name]["params"], name
    assert utils.flow_voxel_batch is flow_voxel.flow_voxel_batch
    lib = _hip.load_library()
    for sym in ("advect", "propagate_bilinear", "truncate_mean"):
        assert all(hasattr(lib, f"ebos_flow_voxel_{sym}_{t}") for t in ("f32", "f64"))
    assert all(hasattr(lib, f"ebos_flow_{s}_step_{t}") for s in ("upwind", "burgers") for t in ("f32", "f64"))
    assert flow_voxel.halo_cap() == 8
