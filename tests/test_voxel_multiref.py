"""CPU checks of the time-aware objective at K reference times: the ``time_aware`` block's new keys, the solver's routing, the argument
validation of the C entry points (before any HIP call: usable without a GPU), the layout of
``ebos_cmax_voxel_multiref_batch_problem`` against its ctypes mirror, what the plan operators refuse and the shipped configuration."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ebos_iwe_voxel_multiref_tiled_f32", "ebos_iwe_voxel_multiref_owner_bwd_f32", "ebos_iwe_voxel_multiref_tiled_batch_f32",
       "ebos_iwe_voxel_multiref_owner_bwd_batch_f32", "ebos_cmax_voxel_multiref_solve_batch_f32",
       "ebos_cmax_voxel_multiref_gradient_batch_f32"]


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


# ---------------------------------------------------------------------------------------------- the block
def test_parse_time_aware_directions_and_normalize():
    from event_based_bos_amd.solver.contrast_maximization import parse_time_aware

    plain = {"time_bin": 5, "scheme": "upwind", "t0_location": "middle", "clamp": None}
    assert parse_time_aware({"time_bin": 5}) == plain                                   # exactly the dict it always was
    assert parse_time_aware({"time_bin": 5, "native": True}) == dict(plain, native=True)
    got = parse_time_aware({"time_bin": 5, "directions": ["first", 0.25, 1]})
    assert got == dict(plain, directions=["first", 0.25, 1.0]) and type(got["directions"][2]) is float and "normalize" not in got
    got = parse_time_aware({"time_bin": 5, "directions": ("first", "middle", "last"), "normalize": True, "native": True})
    assert got == dict(plain, directions=["first", "middle", "last"], normalize=True, native=True)
    assert parse_time_aware({"time_bin": 5, "directions": ["last"], "normalize": False})["normalize"] is False
    for bad in ({"time_bin": 5, "normalize": True}, {"time_bin": 5, "directions": []}, {"time_bin": 5, "directions": ["first"] * 5},
                {"time_bin": 5, "directions": ["first", "random"]}, {"time_bin": 5, "directions": ["sideways"]},
                {"time_bin": 5, "directions": "first"}, {"time_bin": 5, "directions": ["first"], "normalize": "yes"},
                {"time_bin": 5, "directions": ["first"], "normalise": True}, {"time_bin": 5, "directions": [float("nan")]}):
        with pytest.raises(ValueError):
            parse_time_aware(bad)
    with pytest.raises(ValueError, match="directions"):
        parse_time_aware({"time_bin": 5, "normalize": True})


def _config(native=True, **over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": [12, 14], "sliding_window": [12, 14]}, "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}},
           "time_aware": {"time_bin": 5, "scheme": "upwind", "t0_location": "middle", "directions": ["first", "middle", "last"]}}
    if native:
        cfg["time_aware"]["native"] = True
    cfg.update(over)
    return cfg


def test_solver_routes_the_combined_configuration(lib):
    import event_based_bos_amd as ebos

    make = ebos.solver.collections["contrast_maximization"]
    slv = make((37, 70), (37, 70), solver_config=_config())
    assert slv.time_aware["directions"] == ["first", "middle", "last"] and slv.time_aware["native"] is True
    assert slv.multi_reference is None and slv.fused_loop is False and slv.use_graph is False and slv.resident is False
    assert slv._native_batch() and slv.plan_tile() == (64, 64)                          # as time_aware: {native: true} alone
    assert make((37, 70), (37, 70), solver_config=_config(tile=[32, 32])).plan_tile() == (32, 32)
    make((37, 70), (37, 70), solver_config=_config(cost_with_weight={"image_variance": 1.0, "flow_norm": 0.1, "image_gradient": 0.1}))
    scipy = make((37, 70), (37, 70), solver_config=_config(optimizer={"method": "L-BFGS-B", "n_iter": 5}))
    assert not scipy._native_batch()                                                    # a scipy method: window by window
    make((37, 70), (37, 70), solver_config=_config(outer_padding=2))
    # the native family's refusals name the key
    for key, over in (("blur_sigma", dict(iwe={"blur_sigma": 1})), ("cost", dict(cost="gradient_magnitude")),
                      ("optimizer.method", dict(optimizer={"method": "grid", "n_iter": 5})),
                      ("cost_with_weight", dict(cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5}))):
        with pytest.raises(NotImplementedError, match=key) as e:
            make((37, 70), (37, 70), solver_config=_config(**over))
        assert "time_aware.native" in str(e.value)
    # without native the same configurations are the autograd loop's
    slv = make((37, 70), (37, 70), solver_config=_config(native=False, iwe={"blur_sigma": 1},
                                                       cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5}))
    assert not slv._native_batch() and slv.time_aware["directions"] == ["first", "middle", "last"]
    # a multi_reference block beside time_aware stays refused, and says where the directions belong
    with pytest.raises(NotImplementedError, match="time_aware") as e:
        make((37, 70), (37, 70), solver_config=_config(multi_reference={"directions": ["first", "last"]}))
    assert "directions" in str(e.value)
    for model in ("2d-translation", "rigid-optical-flow"):
        with pytest.raises(NotImplementedError, match="motion_model"):
            make((37, 70), (37, 70), solver_config=_config(motion_model=model))
    with pytest.raises(ValueError, match="normalize"):
        make((37, 70), (37, 70), solver_config=_config(time_aware={"time_bin": 5, "normalize": True}))


def test_shipped_configuration_loads(lib):
    import yaml

    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver.contrast_maximization import parse_time_aware

    with open(os.path.join(ROOT, "configs", "cmax_time_aware_multi_reference.yaml")) as f:
        cfg = ebos.utils.propagate_config(yaml.safe_load(f))
    ta = parse_time_aware(cfg["solver"]["time_aware"])
    assert ta["directions"] == ["first", "middle", "last"] and ta["time_bin"] == 5 and ta["native"] is True and ta["normalize"] is True
    assert cfg["solver"]["optimizer"]["method"] == "Adam"
    shape = (cfg["data"]["height"], cfg["data"]["width"])
    slv = ebos.solver.collections[cfg["solver"]["method"]](shape, shape, solver_config=cfg["solver"])
    assert slv._native_batch() and slv.plan_tile() == (64, 64)


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_prototypes_equal_the_ctypes_mirror(lib):
    from event_based_bos_amd import _hip

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebos_hip.h")).read(), flags=re.S)
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


def _c_compiler():
    """A host C compiler: gcc / cc / clang where one is on the path, else the clang that ships beside hipcc -- wherever the library
    can be built there is one, so the layout test does not skip."""
    from event_based_bos_amd.build import hipcc

    for name in ("gcc", "cc", "clang"):
        if shutil.which(name):
            return shutil.which(name)
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc())))
    for rel in ("llvm/bin/clang", "lib/llvm/bin/clang", "bin/amdclang"):
        if os.path.exists(os.path.join(root, rel)):
            return os.path.join(root, rel)
    raise AssertionError("no host C compiler found beside hipcc")


def test_problem_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """``ebos_cmax_voxel_multiref_batch_problem`` as a C compiler lays it out == ``_hip.CmaxVoxelMultirefBatchProblem`` (size and every
    field offset), by the gcc ``offsetof`` method of tests/test_abi.py; the batch problem itself is not grown."""
    from event_based_bos_amd import _hip

    gcc = _c_compiler()
    c_name, mirror = "ebos_cmax_voxel_multiref_batch_problem", _hip.CmaxVoxelMultirefBatchProblem
    fields = [f[0] for f in mirror._fields_]
    hdr = open(os.path.join(ROOT, "include", "ebos_hip.h")).read()
    body = hdr[hdr.index("typedef struct %s {" % c_name):hdr.index("} %s;" % c_name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split("{", 1)[1].split(";"):
        declared += re.findall(r"[*\s,]([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[A-Za-z0-9_]+\])?\s*(?=,|$)", stmt.strip())
    assert declared == fields, (declared, fields)
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ebos_hip.h"', 'int main(void) {',
             '  printf("%%zu\\n", sizeof(%s));' % c_name]
    lines += [f'  printf("%zu\\n", offsetof({c_name}, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]
    # the batch problem's fields without owner_bwd, plus K, shifts, inv_norm and value
    base = [f[0] for f in _hip.CmaxVoxelBatchProblem._fields_]
    assert [f for f in fields if f not in ("K", "shifts", "inv_norm", "value")] == [f for f in base if f != "owner_bwd"]


def _problem(B=3, K=3):
    """A problem whose pointers are non-NULL dummies: validation never dereferences them, and a valid one would need a GPU."""
    from event_based_bos_amd import _hip

    q = _hip.CmaxVoxelMultirefBatchProblem()
    for name, kind in q._fields_:
        if kind is _hip._P:
            setattr(q, name, 0x1000)
    q.B, q.K = B, K
    for k, s in enumerate((0.0, -0.5, -1.0, -0.25)):
        q.shifts[k] = s
    for b in range(B):
        q.n[b] = 100 * b                                   # (the first window is empty: valid)
    q.H, q.W, q.tile_h, q.tile_w, q.halo, q.splits = 37, 70, 32, 32, 32, 1
    q.T, q.scheme, q.t0_index, q.route = 5, _hip.FLOW_UPWIND, 2, _hip.FLOW_ROUTE_AUTO
    q.gh, q.gw, q.patch_h, q.patch_w, q.slide_h, q.slide_w = 4, 5, 12, 14, 12, 14
    q.w_variance, q.lr, q.beta1, q.beta2, q.eps = 1.0, 0.05, 0.9, 0.999, 1e-8
    q.cost_scratch_bytes, q.adjoint_workspace_elems, q.losses_cap = 1 << 24, 1 << 30, 8
    return q


@pytest.mark.parametrize("entry", ["solve", "gradient"])
def test_native_loop_validates_before_any_launch(lib, entry):
    who = b"ebos_cmax_voxel_multiref_%s_batch:" % entry.encode()

    def call(q):
        p = None if q is None else ctypes.byref(q)
        rc = lib.ebos_cmax_voxel_multiref_solve_batch_f32(p, 1, None) if entry == "solve" else \
            lib.ebos_cmax_voxel_multiref_gradient_batch_f32(p, None)
        return rc, lib.ebos_last_error()

    def refused(q, word, want=-1):
        rc, msg = call(q)
        assert rc == want and msg.startswith(who) and word in msg, (rc, msg)

    refused(None, b"NULL problem")
    for K in (0, 5):
        refused(_problem(K=K), b"K = %d is outside [1, 4]" % K)
    for bad in (float("nan"), float("inf")):
        q = _problem()
        q.shifts[1] = bad
        refused(q, b"shifts[1] is not finite")
    q = _problem(K=2)
    q.shifts[3] = float("nan")                              # beyond K: not read
    q.theta = None
    refused(q, b"NULL theta")
    for name in ("inv_norm", "value"):
        q = _problem()
        setattr(q, name, None)
        refused(q, b"NULL inv_norm / value")
    # the scratch of B K images: what suffices for the B windows of one reference time does not
    q = _problem()
    q.cost_scratch_bytes = lib.ebos_cost_scratch_bytes(3 * 3) - 1
    assert lib.ebos_cost_scratch_bytes(3) <= q.cost_scratch_bytes
    refused(q, b"cost_scratch too small for 3 windows x 3 reference times", want=-4)
    q = _problem()
    q.cost_scratch_bytes = lib.ebos_cost_scratch_bytes(3 * 3)
    q.iwe = None
    refused(q, b"NULL image / scratch buffer")
    # ... plus everything the batch loop refuses
    for field, value, word in (("B", 0, b"B = 0"), ("B", 65, b"B = 65"), ("T", 0, b"outside [1, 255]"), ("T", 256, b"outside [1, 255]"),
                               ("scheme", 2, b"scheme 2"), ("t0_index", 5, b"t0_index"), ("xs", None, b"NULL plan buffer"),
                               ("key_offsets", None, b"NULL plan buffer"), ("w_variance", 0.0, b"w_variance"), ("splits", 0, b"bad sizes")):
        q = _problem()
        setattr(q, field, value)
        refused(q, word)
    q = _problem()
    q.has_clamp, q.voxel_clamped = 1, None
    refused(q, b"has_clamp")
    q = _problem()
    q.w_flow_norm, q.d_reg = 0.1, None
    refused(q, b"d_reg")
    q = _problem()
    q.n[1] = -1
    refused(q, b"n = -1")
    if entry == "solve":
        assert lib.ebos_cmax_voxel_multiref_solve_batch_f32(ctypes.byref(_problem()), -1, None) == -1
        assert b"negative n_iter" in lib.ebos_last_error()
        q = _problem()                                      # exactly the scratch of B K images and no iterations: nothing is launched
        q.cost_scratch_bytes = lib.ebos_cost_scratch_bytes(3 * 3)
        assert lib.ebos_cmax_voxel_multiref_solve_batch_f32(ctypes.byref(q), 0, None) == 0


def test_kernel_entries_validate_before_any_launch(lib):
    p = 0x1000
    sh = (ctypes.c_float * 4)(0.0, -0.5, -1.0, -0.25)
    ns = (ctypes.c_int64 * 2)(10, 0)
    fwd = dict(xs=p, ys=p, dts=p, bins=p, key_offsets=p, n=10, voxel=p, T=5, H=37, W=70, tile_h=32, tile_w=32, halo=32, splits=1,
               pad_h=0, pad_w=0, shifts=sh, K=3, iwes=p, stream=None)
    bwd = dict(xs=p, ys=p, dts=p, bins=p, key_offsets=p, n=10, voxel=p, T=5, H=37, W=70, tile_h=32, tile_w=32, pad_h=0, pad_w=0,
               shifts=sh, K=3, g_images=p, affine=None, g_lo=0, d_voxel=p, stream=None)

    def batch(args):
        a = dict(args)
        out = {}
        for k, v in a.items():
            if k == "n":
                out["ns"], out["B"] = ns, 2
            else:
                out[k] = v
        return out

    for fn, who, args in ((lib.ebos_iwe_voxel_multiref_tiled_f32, b"ebos_iwe_voxel_multiref_tiled:", fwd),
                          (lib.ebos_iwe_voxel_multiref_owner_bwd_f32, b"ebos_iwe_voxel_multiref_owner_bwd:", bwd),
                          (lib.ebos_iwe_voxel_multiref_tiled_batch_f32, b"ebos_iwe_voxel_multiref_tiled_batch:", batch(fwd)),
                          (lib.ebos_iwe_voxel_multiref_owner_bwd_batch_f32, b"ebos_iwe_voxel_multiref_owner_bwd_batch:", batch(bwd))):
        def refused(word, **over):
            rc = fn(*dict(args, **over).values())
            msg = lib.ebos_last_error()
            assert rc == -1 and msg.startswith(who) and word in msg, (rc, msg)

        refused(b"K = 0", K=0)
        refused(b"K = 5", K=5)
        refused(b"shifts is NULL", shifts=None)
        refused(b"shifts[2] is not finite", shifts=(ctypes.c_float * 4)(0.0, -0.5, float("nan"), 0.0))
        refused(b"outside [1, 255]", T=0)
        refused(b"outside [1, 255]", T=256)
        refused(b"NULL", voxel=None)
        refused(b"NULL", key_offsets=None)
        refused(b"NULL event buffer", bins=None)
        refused(b"bad sizes", tile_h=0)
        if "B" in args:
            refused(b"B = 0", B=0)
            refused(b"B = 65", B=65)
            refused(b"n = -1", ns=(ctypes.c_int64 * 2)(10, -1))
        else:
            refused(b"n = -1", n=-1)
    # an empty window adds nothing to its images: nothing is launched
    assert lib.ebos_iwe_voxel_multiref_tiled_f32(*dict(fwd, n=0, xs=None, ys=None, dts=None, bins=None).values()) == 0


# ---------------------------------------------------------------------------------------------- the plan operators
def test_canonical_stack_orders_every_run_alike():
    """``TimeAwarePlanStack.canonical``: whatever order a build leaves inside a source pixel's run, the canonical streams are the same
    (sorted by (dt, x, y, bin) inside every run); the runs themselves, the offsets and the counts do not change."""
    from event_based_bos_amd.event_plan import TimeAwarePlanStack

    def stack(x, y, dt, bins, ko):
        st = object.__new__(TimeAwarePlanStack)
        st.x, st.y, st.dt, st.bins, st.key_offsets, st.n, st.ns, st.plans, st.perm = x, y, dt, bins, ko, len(x), [20, 30], [], None
        return st

    g = torch.Generator().manual_seed(0)
    n = 50
    ko = torch.tensor([[0, 3, 3, 10, 20], [20, 25, 40, 40, 50]], dtype=torch.int32)      # two windows, an empty run in each
    x, y = torch.rand(n, generator=g), torch.rand(n, generator=g)
    dt = torch.randint(0, 4, (n,), generator=g).float()                                   # ties in dt: x decides
    bins = torch.randint(0, 3, (n,), generator=g, dtype=torch.uint8)
    first = stack(x, y, dt, bins, ko).canonical()
    assert first.canonical() is first and first.key_offsets is ko and first.ns == [20, 30] and not hasattr(first, "perm")
    flat = ko.reshape(-1).tolist()
    for a, b in zip(flat[:-1], flat[1:]):
        want = sorted(zip(dt[a:b].tolist(), x[a:b].tolist(), y[a:b].tolist(), bins[a:b].tolist()))
        assert want == list(zip(first.dt[a:b].tolist(), first.x[a:b].tolist(), first.y[a:b].tolist(), first.bins[a:b].tolist()))
    shuffle = torch.arange(n)
    for a, b in zip(flat[:-1], flat[1:]):
        if b > a:
            shuffle[a:b] = a + torch.randperm(b - a, generator=g)
    second = stack(x[shuffle], y[shuffle], dt[shuffle], bins[shuffle], ko).canonical()
    assert not torch.equal(x[shuffle], x) and all(torch.equal(getattr(first, k), getattr(second, k)) for k in ("x", "y", "dt", "bins"))


def _cpu_plan(n=12, tile=(32, 32), shape=(37, 70), fraction=0.0, normalized=True, binned=True, bins=True):
    """An ``EventPlan`` of CPU tensors (tests/test_multiref.py): the operators' refusals come before any launch."""
    from event_based_bos_amd.event_plan import EventPlan

    n_keys = -(-shape[0] // tile[0]) * -(-shape[1] // tile[1]) * tile[0] * tile[1]
    ko = torch.clamp(torch.arange(n_keys + 1, dtype=torch.int32), max=n) if binned else None
    f = lambda: torch.arange(n, dtype=torch.float32)  # noqa: E731
    return EventPlan(f(), f(), f(), f(), shape, n, n, tile if binned else None, ko, None, dt_bound=1.0, ref_fraction=fraction,
                     normalized_t=normalized, bins=torch.zeros(n, dtype=torch.uint8) if bins else None, time_bin=5 if bins else None)


def test_plan_operators_refuse_before_any_launch(lib):
    vox = torch.zeros((5, 2, 37, 70))
    for call in (lambda p, d, v=vox: p.iwe_voxel_multi(v, d), lambda p, d, v=vox: p.contrast_voxel_multi(v, d),
                 lambda p, d, v=vox: p.variance_voxel_multi_value_and_grad(v, d)):
        plan = _cpu_plan()
        for bad in ([], ["first"] * 5, ["first", "random"], "first", ["sideways"]):
            with pytest.raises(ValueError):
                call(plan, bad)
        with pytest.raises(ValueError, match="normalised time"):
            call(_cpu_plan(normalized=False), ["first", "last"])
        with pytest.raises(ValueError, match="reference fraction"):
            call(_cpu_plan(fraction=None), ["first", "last"])
        with pytest.raises(ValueError, match="time bins"):
            call(_cpu_plan(bins=False), ["first", "last"])
        with pytest.raises(NotImplementedError, match="binned"):
            call(_cpu_plan(binned=False), ["first", "last"])
        plan = _cpu_plan()
        plan.__dict__["_deferred"] = True
        with pytest.raises(NotImplementedError, match="deferred=True"):
            call(plan, ["first", "last"])
        with pytest.raises(ValueError, match="time_bin=5"):
            call(_cpu_plan(), ["first", "last"], torch.zeros((4, 2, 37, 70)))
        with pytest.raises(ValueError, match="voxel must be"):
            call(_cpu_plan(), ["first", "last"], torch.zeros((5, 2, 37, 71)))
    with pytest.raises(KeyError):
        _cpu_plan().contrast_voxel_multi(vox, ["first"], cost="sharpness")
