"""CPU checks of the multi-reference contrast's boundary: the argument validation of ``ebos_iwe_dense_multiref_tiled_f32`` and
``ebos_iwe_dense_multiref_owner_bwd_f32`` (before any HIP call: usable without a GPU), ``ebos_iwe_multiref_fits``, the header
prototypes against the ctypes mirror, the ``multi_reference`` block, the refusals of the plan operators and the solver that need no
device, and the host-side shifts f - r_k."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ebos_iwe_multiref_fits", "ebos_iwe_dense_multiref_tiled_f32", "ebos_iwe_dense_multiref_owner_bwd_f32")


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


def _shifts(*v):
    return (ctypes.c_float * len(v))(*v)


def test_tiled_forward_validates_before_any_launch(lib):
    p = 0x1000
    args = dict(xs=p, ys=p, dts=p, key_offsets=p, n=10, flow=p, H=37, W=70, tile_h=32, tile_w=32, halo=8, splits=1, pad_h=0, pad_w=0,
                shifts=_shifts(0.0, -0.5, -1.0), K=3, iwes=p, stream=None)

    def call(**over):
        return lib.ebos_iwe_dense_multiref_tiled_f32(*dict(args, **over).values())

    assert call(key_offsets=None) == -1 and b"key_offsets is NULL" in lib.ebos_last_error()       # an un-binned plan
    assert call(flow=None) == -1 and b"NULL flow/iwes" in lib.ebos_last_error()
    assert call(iwes=None) == -1 and call(xs=None) == -1 and call(dts=None) == -1
    for K in (0, 5, -1):
        assert call(K=K) == -1 and b"outside [1, 4]" in lib.ebos_last_error()
    assert call(shifts=None) == -1 and b"shifts is NULL" in lib.ebos_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(shifts=_shifts(0.0, bad, 1.0)) == -1 and b"shifts[1] is not finite" in lib.ebos_last_error()
    assert call(H=0) == -1 and call(splits=0) == -1 and call(splits=65) == -1 and call(pad_h=-1) == -1 and call(n=-1) == -1
    assert b"bad sizes" in lib.ebos_last_error()
    # K windows that do not fit, and a tile that is no tiled configuration: an error, not a launch (-3 = EBOS_ERR_UNSUPPORTED)
    assert call(tile_h=64, tile_w=64, halo=64, K=2, shifts=_shifts(0.0, 1.0)) == -3 and b"do not fit" in lib.ebos_last_error()
    assert call(tile_h=33, tile_w=32) == -3
    # a shift beyond the K given is not read
    assert call(shifts=_shifts(0.25), K=1, tile_h=33) == -3


def test_owner_backward_validates_before_any_launch(lib):
    p = 0x1000
    args = dict(xs=p, ys=p, dts=p, key_offsets=p, n=10, flow=p, H=37, W=70, tile_h=32, tile_w=32, pad_h=0, pad_w=0,
                shifts=_shifts(0.0, -0.5, -1.0), K=3, g_images=p, affine=None, g_lo=0, d_flow=p, stream=None)

    def call(**over):
        return lib.ebos_iwe_dense_multiref_owner_bwd_f32(*dict(args, **over).values())

    assert call(key_offsets=None) == -1 and b"key_offsets is NULL" in lib.ebos_last_error()
    assert call(d_flow=None) == -1 and b"NULL flow/g_images/d_flow" in lib.ebos_last_error()
    assert call(g_images=None) == -1 and call(flow=None) == -1 and call(ys=None) == -1
    assert call(K=0) == -1 and b"outside [1, 4]" in lib.ebos_last_error()
    assert call(K=5) == -1
    assert call(shifts=None) == -1 and b"shifts is NULL" in lib.ebos_last_error()
    assert call(shifts=_shifts(float("nan"), 0.0, 0.0)) == -1 and b"shifts[0] is not finite" in lib.ebos_last_error()
    assert call(tile_h=0) == -1 and call(g_lo=-1) == -1 and call(W=0) == -1 and call(n=2 ** 31) == -1
    assert b"bad sizes" in lib.ebos_last_error()


def test_fits_follows_the_accumulator_rule(lib):
    from event_based_bos_amd import _hip

    fits = lib.ebos_iwe_multiref_fits
    for th, tw, hl in _hip.tiled_configs():
        got = [fits(th, tw, hl, K) for K in (1, 2, 3, 4)]
        assert all(a >= b for a, b in zip(got, got[1:])), (th, tw, hl, got)              # it never grows with K
        cells = (th + 2 * hl) * (tw + 2 * hl)
        want = [2 if cells * K * 8 <= 160 * 1024 else (1 if cells * K * 4 <= 160 * 1024 else 0) for K in (1, 2, 3, 4)]
        assert got == want and got[0] != 0
        assert fits(th, tw, hl, 0) == 0 and fits(th, tw, hl, 5) == 0
    assert fits(64, 64, 64, 2) == 0
    assert fits(33, 32, 8, 1) == 0 and fits(32, 32, 7, 1) == 0 and fits(0, 32, 8, 1) == 0   # no tiled configuration
    assert fits(32, 32, 8, 4) != 0
    assert fits(32, 32, 32, 3) == 1
    assert all(fits(64, 64, 16, K) != 0 for K in (1, 2, 3, 4))                             # the solver's default tile


def test_header_prototypes_equal_the_ctypes_mirror(lib):
    from event_based_bos_amd import _hip

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebos_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+EBOS_MULTIREF_MAX\s+4\b", hdr) and _hip.MULTIREF_MAX == 4
    assert re.search(r"#define\s+EBOS_ABI_VERSION\s+2\b", hdr) and _hip.ABI_VERSION == 2 and lib.ebos_version() == 2
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        res, mirror = _hip.SIGNATURES[name]
        assert res is ctypes.c_int
        params = [" ".join(q.split()) for q in m.group(1).split(",")]
        assert len(params) == len(mirror), name
        for decl, ct in zip(params, mirror):
            if "*" in decl or decl.startswith("ebos_stream_t"):
                assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, decl, ct)
                if issubclass(ct, ctypes._Pointer):                                       # a typed host pointer: the header's type
                    assert ct._type_ is ctypes.c_float and decl.startswith("const float*"), (name, decl)
            elif decl.startswith("int64_t "):
                assert ct is ctypes.c_int64, (name, decl)
            else:
                assert decl.startswith("int ") and ct is ctypes.c_int, (name, decl)
        assert hasattr(lib, name)


def test_parse_multi_reference_block():
    from event_based_bos_amd.solver.contrast_maximization import parse_multi_reference

    assert parse_multi_reference(None) is None
    assert parse_multi_reference({"directions": ["first", "middle", "last"]}) == \
        {"directions": ["first", "middle", "last"], "normalize": False, "fused": None}
    got = parse_multi_reference({"directions": ["first", 0.25, 1], "normalize": True, "fused": False})
    assert got == {"directions": ["first", 0.25, 1.0], "normalize": True, "fused": False} and type(got["directions"][2]) is float
    for bad in ({"directions": ["first"], "normalise": True}, {"normalize": True}, {"directions": []},
                {"directions": ["first"] * 5}, {"directions": ["first", "random"]}, {"directions": ["sideways"]},
                {"directions": "first"}, {"directions": ["first"], "normalize": "yes"}, {"directions": ["first"], "fused": 1}):
        with pytest.raises(ValueError):
            parse_multi_reference(bad)


def _config(**over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": [12, 14], "sliding_window": [12, 14]}, "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}},
           "multi_reference": {"directions": ["first", "middle", "last"]}}
    cfg.update(over)
    return cfg


def test_solver_takes_the_block_and_refuses_what_is_outside(lib):
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver import WindowPipeline

    make = ebos.solver.collections["contrast_maximization"]
    slv = make((37, 70), (37, 70), solver_config=_config())
    assert slv.multi_reference == {"directions": ["first", "middle", "last"], "normalize": False, "fused": None}
    assert slv.fused_loop is False and slv.use_graph is False and slv.resident is False
    assert slv.plan_tile() == (64, 64)
    assert make((37, 70), (37, 70), solver_config=_config(tile=[32, 32])).plan_tile() == (32, 32)
    make((37, 70), (37, 70), solver_config=_config(optimizer={"method": "L-BFGS-B", "n_iter": 5}))
    make((37, 70), (37, 70), solver_config=_config(iwe={"blur_sigma": 1}, cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5,
                                                                                           "flow_norm": 0.1}))
    with pytest.raises(NotImplementedError, match="time_aware"):
        make((37, 70), (37, 70), solver_config=_config(time_aware={"time_bin": 5}))
    for model in ("2d-translation", "rigid-optical-flow"):
        with pytest.raises(NotImplementedError, match="motion_model"):
            make((37, 70), (37, 70), solver_config=_config(motion_model=model))
    with pytest.raises(ValueError, match="unknown key"):
        make((37, 70), (37, 70), solver_config=_config(multi_reference={"directions": ["first"], "direction": "last"}))
    with pytest.raises(NotImplementedError, match="multi_reference"):
        WindowPipeline(slv)
    # without the block nothing changes
    plain = _config()
    plain.pop("multi_reference")
    slv = make((37, 70), (37, 70), solver_config=plain)
    assert slv.multi_reference is None and slv.fused_loop is True and slv.use_graph is True and slv.plan_tile() != (64, 64)


def _cpu_plan(n=12, tile=(32, 32), shape=(37, 70), fraction=0.0, normalized=True, binned=True):
    """An ``EventPlan`` of CPU tensors (tests/test_voxel_loop_batch.py): the operators' refusals come before any launch."""
    from event_based_bos_amd.event_plan import EventPlan

    n_keys = -(-shape[0] // tile[0]) * -(-shape[1] // tile[1]) * tile[0] * tile[1]
    ko = torch.clamp(torch.arange(n_keys + 1, dtype=torch.int32), max=n) if binned else None
    f = lambda: torch.arange(n, dtype=torch.float32)  # noqa: E731
    return EventPlan(f(), f(), f(), f(), shape, n, n, tile if binned else None, ko, None, dt_bound=1.0, ref_fraction=fraction,
                     normalized_t=normalized)


def test_plan_operators_refuse_before_any_launch(lib):
    flow = torch.zeros((2, 37, 70))
    plan = _cpu_plan()
    for op in (plan.iwe_dense_multi, plan.contrast_dense_multi):
        for bad in ([], ["first"] * 5, ["first", "random"], ["sideways"], "first", None):
            with pytest.raises(ValueError):
                op(flow, bad)
        with pytest.raises(ValueError, match="normalised time"):
            getattr(_cpu_plan(normalized=False), op.__name__)(flow, ["first", "last"])
        with pytest.raises(ValueError, match="reference fraction"):
            getattr(_cpu_plan(fraction=None), op.__name__)(flow, ["first", "last"])
        with pytest.raises(NotImplementedError, match="binned"):
            getattr(_cpu_plan(binned=False), op.__name__)(flow, ["first", "last"])
        deferred = _cpu_plan()
        deferred.__dict__["_deferred"] = True
        with pytest.raises(NotImplementedError, match="deferred=True"):
            getattr(deferred, op.__name__)(flow, ["first", "last"])
        lean = _cpu_plan()
        lean.x = lean.y = lean.dt = lean.p = None
        lean.cpix = torch.zeros(4, dtype=torch.int16)
        with pytest.raises(NotImplementedError, match="lean plan"):
            getattr(lean, op.__name__)(flow, ["first", "last"])
        with pytest.raises(ValueError, match="fused"):
            op(flow, ["first", "last"], fused="yes")
    with pytest.raises(KeyError):
        plan.contrast_dense_multi(flow, ["first"], cost="sharpness")
    # fused=True where no built halo of the tile keeps K windows: an error that names the way out
    with pytest.raises(NotImplementedError, match="fused=False"):
        _cpu_plan(tile=(48, 48)).iwe_dense_multi(flow, ["first", "last"], fused=True)


def test_host_side_shifts_and_routes(lib):
    from event_based_bos_amd import event_plan as EP

    f32 = lambda v: float(np.float32(v))  # noqa: E731
    dirs = ["first", 0.25, "middle", "last"]
    assert EP.multi_reference_fractions(dirs) == [0.0, 0.25, 0.5, 1.0]
    assert EP.multi_reference_fractions(["before", "after"]) == [-1.0, 2.0]
    assert EP.multi_reference_shifts(_cpu_plan(fraction=0.0), dirs) == [0.0, -0.25, -0.5, -1.0]                 # a 'first' plan
    assert EP.multi_reference_shifts(_cpu_plan(fraction=0.5), dirs) == [0.5, 0.25, 0.0, -0.5]                   # 'middle'
    assert EP.multi_reference_shifts(_cpu_plan(fraction=0.25), dirs) == [0.25, 0.0, -0.25, -0.75]               # 0.25
    assert EP.multi_reference_shifts(_cpu_plan(fraction=0.0), ["before", "middle", "after"]) == [1.0, -0.5, -2.0]
    assert EP.multi_reference_shifts(_cpu_plan(fraction=0.3), [0.1]) == [f32(0.3 - 0.1)]                        # rounded to float32 once
    # the builders' record of the fraction
    assert EP.ref_fraction_for("first") == 0.0 and EP.ref_fraction_for("middle") == 0.5 and EP.ref_fraction_for("last") == 1.0
    assert EP.ref_fraction_for("before") == -1.0 and EP.ref_fraction_for("after") == 2.0 and EP.ref_fraction_for(0.25) == 0.25
    assert EP.ref_fraction_for("random") is None
    # routes: the halo asked for where K windows of it fit, else (fused=True) the largest built halo that does; fused=None takes the
    # loop route where nothing fits
    job = EP._multiref_job(_cpu_plan(), dirs[:3], (0, 0), 32, None, True, "t")
    assert job.fused and job.halo == 32 and job.shifts == (0.0, -0.25, -0.5) and job.pad == (0, 0)
    job = EP._multiref_job(_cpu_plan(tile=(64, 64)), dirs[:3], (2, 2), 64, None, True, "t")
    assert job.fused and job.halo == 16 and job.pad == (2, 2)
    job = EP._multiref_job(_cpu_plan(tile=(64, 64)), dirs[:3], (0, 0), 64, None, None, "t")
    assert not job.fused and job.halo == 64
    job = EP._multiref_job(_cpu_plan(), dirs, (0, 0), 8, None, False, "t")
    assert not job.fused and job.halo == 8
    job = EP._multiref_job(_cpu_plan(), dirs, (0, 0), 32, None, None, "t")
    assert job.fused is EP.MULTIREF_DEFAULT_FUSED and job.halo == 32
