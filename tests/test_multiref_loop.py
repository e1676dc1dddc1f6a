"""CPU checks of the K-image slab pipeline and the native multi-reference loop: argument validation of every new entry point
(before any HIP call: usable without a GPU), the header prototypes and the problem struct against the ctypes mirror, the workspace
size, the ``native`` key of the ``multi_reference`` block, the solver's construction and refusals, and the ``fused="slab"`` refusals
of the plan operators."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebos_hip.h")
NEW = ("ebos_slab_multiref_config", "ebos_iwe_slab_multiref_workspace_bytes", "ebos_iwe_dense_slab_multiref_f32",
       "ebos_iwe_dense_tiled_multiref_bwd_f32", "ebos_cmax_multiref_solve_f32", "ebos_cmax_multiref_gradient_f32")
REQUIRED_TRIPLES = ((32, 32, 8), (32, 32, 32), (64, 64, 16))


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


def _shifts(*v):
    return (ctypes.c_float * len(v))(*v)


# ---------------------------------------------------------------------------------------------- validation before any launch
def test_slab_forward_validates_before_any_launch(lib):
    p = 0x1000
    need = lib.ebos_iwe_slab_multiref_workspace_bytes(3, 37, 70, 32, 32, 8, 1, 0, 0)
    args = dict(xs=p, ys=p, dts=p, key_offsets=p, n=10, flow=p, H=37, W=70, tile_h=32, tile_w=32, halo=8, splits=1, pad_h=0, pad_w=0,
                shifts=_shifts(0.0, -0.5, -1.0), K=3, workspace=p, workspace_bytes=need, iwes=p, want_variance=1, omit_boundary=0,
                variances=p, moments=p, stream=None)

    def call(**over):
        return lib.ebos_iwe_dense_slab_multiref_f32(*dict(args, **over).values())

    assert call(flow=None) == -1 and b"NULL flow/iwes/key_offsets/workspace" in lib.ebos_last_error()
    assert call(iwes=None) == -1 and call(key_offsets=None) == -1 and call(workspace=None) == -1
    assert call(xs=None) == -1 and b"NULL event buffer" in lib.ebos_last_error()
    assert call(ys=None) == -1 and call(dts=None) == -1
    for K in (0, 5):
        assert call(K=K) == -1 and b"outside [1, 4]" in lib.ebos_last_error()
    assert call(shifts=None) == -1 and b"shifts is NULL" in lib.ebos_last_error()
    assert call(shifts=_shifts(0.0, float("nan"), 1.0)) == -1 and b"shifts[1] is not finite" in lib.ebos_last_error()
    assert call(H=0) == -1 and call(splits=65) == -1 and call(pad_w=-1) == -1 and call(n=-1) == -1 and b"bad sizes" in lib.ebos_last_error()
    assert call(want_variance=3) == -1
    assert call(variances=None, moments=None) == -1 and b"without an output" in lib.ebos_last_error()
    # what is not built: an error, not a launch (-3 = EBOS_ERR_UNSUPPORTED)
    assert call(tile_h=33) == -3 and b"no kernel built for tile 33x32 halo 8" in lib.ebos_last_error()
    assert call(tile_h=45, tile_w=80, halo=32) == -3 and b"ebos_slab_multiref_config" in lib.ebos_last_error()
    assert call(splits=0) == -3 and b"adaptive work items" in lib.ebos_last_error()
    assert call(halo=lib.ebos_halo_auto(32, 1.0)) == -3 and b"run-time halo windows" in lib.ebos_last_error()
    # a workspace that is too small (-4 = EBOS_ERR_SCRATCH)
    assert call(workspace_bytes=need - 1) == -4 and b"workspace too small" in lib.ebos_last_error()
    assert call(K=4, shifts=_shifts(0.0, 0.1, 0.2, 0.3)) == -4                              # sized for K = 3


def test_tiled_backward_validates_before_any_launch(lib):
    p = 0x1000
    args = dict(xs=p, ys=p, dts=p, key_offsets=p, n=10, flow=p, H=37, W=70, tile_h=32, tile_w=32, halo=8, pad_h=0, pad_w=0,
                shifts=_shifts(0.0, -0.5, -1.0), K=3, g_images=p, affine=None, g_lo=0, var_moments=None, upstream=None, scales=None,
                addend=None, d_flow=p, stream=None)

    def call(**over):
        return lib.ebos_iwe_dense_tiled_multiref_bwd_f32(*dict(args, **over).values())

    assert call(d_flow=None) == -1 and b"NULL flow/g_images/d_flow/key_offsets" in lib.ebos_last_error()
    assert call(g_images=None) == -1 and call(flow=None) == -1 and call(key_offsets=None) == -1 and call(ys=None) == -1
    assert call(var_moments=p) == -1 and b"come together" in lib.ebos_last_error()
    assert call(upstream=p) == -1
    assert call(var_moments=p, upstream=p, affine=p) == -1 and b"exclude each other" in lib.ebos_last_error()
    for K in (0, 5):
        assert call(K=K) == -1 and b"outside [1, 4]" in lib.ebos_last_error()
    assert call(shifts=None) == -1 and b"shifts is NULL" in lib.ebos_last_error()
    assert call(scales=_shifts(1.0, float("inf"), 1.0)) == -1 and b"scales[1] is not finite" in lib.ebos_last_error()
    assert call(W=0) == -1 and call(g_lo=-1) == -1 and call(n=2 ** 31) == -1 and b"bad sizes" in lib.ebos_last_error()
    assert call(tile_w=33) == -3 and b"no kernel built" in lib.ebos_last_error()
    assert call(halo=16) == -3                                                             # (32, 32, 16) is a slab triple, not one of these
    assert call(halo=lib.ebos_halo_auto(32, 1.0)) == -3 and b"run-time halo windows" in lib.ebos_last_error()


def _problem(lib, **over):
    from event_based_bos_amd import _hip

    p = 0x1000
    q = _hip.CmaxMultirefProblem()
    for name in ("xs", "ys", "dts", "key_offsets", "theta", "d_theta", "exp_avg", "exp_avg_sq", "step", "dense", "d_dense", "d_reg", "iwes",
                 "variances", "contrast", "moments", "upstream", "workspace", "reg_partials", "upsample_scratch", "losses"):
        setattr(q, name, p)
    q.n, q.H, q.W, q.tile_h, q.tile_w, q.halo, q.splits, q.K = 10, 37, 70, 32, 32, 8, 1, 3
    q.shifts[0], q.shifts[1], q.shifts[2] = 0.0, -0.5, -1.0
    q.gh, q.gw, q.patch_h, q.patch_w, q.slide_h, q.slide_w = 4, 5, 12, 14, 12, 14
    q.w_variance, q.norm, q.lr, q.beta1, q.beta2, q.eps = 1.0, 1.0, 0.05, 0.9, 0.999, 1e-8
    q.workspace_bytes = lib.ebos_iwe_slab_multiref_workspace_bytes(3, 37, 70, 32, 32, 8, 1, 0, 0)
    q.upsample_scratch_bytes = lib.ebos_upsample_bwd_scratch_bytes(4, 70)
    q.losses_cap = 8
    for k, v in over.items():
        setattr(q, k, v)
    return q


@pytest.mark.parametrize("entry", ["solve", "gradient"])
def test_native_loop_validates_before_any_launch(lib, entry):
    def call(**over):
        q = _problem(lib, **over)
        if entry == "solve":
            return lib.ebos_cmax_multiref_solve_f32(ctypes.byref(q), 2, None)
        return lib.ebos_cmax_multiref_gradient_f32(ctypes.byref(q), None)

    who = b"ebos_cmax_multiref_" + entry.encode()
    fn = lib.ebos_cmax_multiref_solve_f32 if entry == "solve" else lib.ebos_cmax_multiref_gradient_f32
    assert (fn(None, 2, None) if entry == "solve" else fn(None, None)) == -1 and b"NULL problem" in lib.ebos_last_error()
    assert call(theta=None) == -1 and who in lib.ebos_last_error() and b"NULL theta" in lib.ebos_last_error()
    assert call(step=None) == -1 and call(xs=None) == -1 and b"NULL plan buffer" in lib.ebos_last_error()
    for name in ("dense", "d_dense", "iwes", "variances", "moments", "contrast", "upstream", "workspace", "reg_partials", "upsample_scratch"):
        assert call(**{name: None}) == -1 and b"NULL image / scratch buffer" in lib.ebos_last_error(), name
    assert call(d_reg=None, w_flow_norm=0.1) == -1 and b"d_reg is NULL" in lib.ebos_last_error()
    for K in (0, 5):
        assert call(K=K) == -1 and b"outside [1, 4]" in lib.ebos_last_error()
    assert call(w_variance=0.0) == -1 and call(norm=0.0) == -1 and call(norm=float("nan")) == -1 and b"norm" in lib.ebos_last_error()
    assert call(H=0) == -1 and call(gh=0) == -1 and call(steps_done=-1) == -1
    assert call(tile_h=45, tile_w=80, halo=32) == -3 and b"ebos_slab_multiref_config" in lib.ebos_last_error()
    assert call(splits=0) == -3 and call(halo=-(32 + 256 * 64)) == -3
    assert call(workspace_bytes=1024) == -4 and b"workspace too small" in lib.ebos_last_error()
    assert call(upsample_scratch_bytes=0) == -4 and b"upsample_scratch too small" in lib.ebos_last_error()
    if entry == "solve":
        assert lib.ebos_cmax_multiref_solve_f32(ctypes.byref(_problem(lib)), -1, None) == -1 and b"negative n_iter" in lib.ebos_last_error()
        assert lib.ebos_cmax_multiref_solve_f32(ctypes.byref(_problem(lib)), 0, None) == 0   # nothing to enqueue: no device needed


# ---------------------------------------------------------------------------------------------- the ABI
def test_header_prototypes_equal_the_ctypes_mirror(lib):
    from event_based_bos_amd import _hip

    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        res, mirror = _hip.SIGNATURES[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t), name
        params = [" ".join(q.split()) for q in m.group(2).split(",")]
        assert len(params) == len(mirror), name
        for decl, ct in zip(params, mirror):
            if "*" in decl or decl.startswith("ebos_stream_t"):
                assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, decl, ct)
                if issubclass(ct, ctypes._Pointer):                                        # a typed host pointer: the header's type
                    want = {ctypes.c_float: "const float*", ctypes.c_int: "int*"}[ct._type_]
                    assert decl.startswith(want), (name, decl)
            elif decl.startswith("int64_t "):
                assert ct is ctypes.c_int64, (name, decl)
            elif decl.startswith("size_t "):
                assert ct is ctypes.c_size_t, (name, decl)
            else:
                assert decl.startswith("int ") and ct is ctypes.c_int, (name, decl)
        assert hasattr(lib, name)


def test_problem_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """``ebos_cmax_multiref_problem`` as gcc lays it out == ``_hip.CmaxMultirefProblem`` (size and every field offset), by the method
    of tests/test_abi.py; the struct is also part of a C99 -pedantic -Werror syntax check of the header."""
    from event_based_bos_amd import _hip

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    c_name, mirror = "ebos_cmax_multiref_problem", _hip.CmaxMultirefProblem
    fields = [f[0] for f in mirror._fields_]
    hdr = open(HEADER).read()
    body = hdr[hdr.index("typedef struct %s {" % c_name):hdr.index("} %s;" % c_name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"\[[^\]]*\]", "", body)                                                 # (an array member is declared by its name)
    declared = []
    for stmt in body.split("{", 1)[1].split(";"):
        declared += re.findall(r"[*\s,]([A-Za-z_][A-Za-z0-9_]*)\s*(?=,|$)", stmt.strip())
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
    want = [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]
    assert got == want
    assert mirror.shifts.size == 4 * _hip.MULTIREF_MAX
    chk = tmp_path / "hdr.c"
    chk.write_text('#include "ebos_hip.h"\nint main(void) { ebos_cmax_multiref_problem p; p.K = EBOS_MULTIREF_MAX; p.shifts[p.K - 1] = 0.0f; '
                   '(void)p; return 0; }\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        str(chk)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_workspace_bytes_and_built_triples(lib):
    from event_based_bos_amd import _hip

    built = _hip.slab_multiref_configs()
    assert all(t in built for t in REQUIRED_TRIPLES) and all(len(t) == 3 for t in built)
    assert lib.ebos_slab_multiref_config(None, 0) == len(built)
    slab = set(_hip.slab_configs())
    assert all(t in slab for t in built)                                                   # every triple is one of the single form's
    size = lib.ebos_iwe_slab_multiref_workspace_bytes
    for th, tw, hl in built:
        for (H, W), splits, pad in (((37, 70), 1, 0), ((37, 70), 3, 2), ((260, 346), 1, 0), ((720, 1280), 2, 0)):
            got = [size(K, H, W, th, tw, hl, splits, pad, pad) for K in (1, 2, 3, 4)]
            assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])), (th, tw, hl, got)
            assert got[0] >= lib.ebos_iwe_slab_workspace_bytes(H, W, th, tw, hl, splits, pad, pad)
    assert size(0, 37, 70, 32, 32, 8, 1, 0, 0) == 0 and size(5, 37, 70, 32, 32, 8, 1, 0, 0) == 0
    assert size(3, 37, 70, 33, 32, 8, 1, 0, 0) == 0 and size(3, 37, 70, 32, 32, 8, 0, 0, 0) == 0 and size(3, 0, 70, 32, 32, 8, 1, 0, 0) == 0


# ---------------------------------------------------------------------------------------------- the block and the solver
def test_parse_multi_reference_native_key():
    from event_based_bos_amd.solver.contrast_maximization import parse_multi_reference

    base = {"directions": ["first", "middle", "last"]}
    assert parse_multi_reference(base) == {"directions": ["first", "middle", "last"], "normalize": False, "fused": None}   # absent: three keys
    assert parse_multi_reference(dict(base, native=True)) == {"directions": ["first", "middle", "last"], "normalize": False, "fused": None,
                                                               "native": True}
    assert parse_multi_reference(dict(base, native=False))["native"] is False
    for bad in ("yes", 1, None, "true"):
        with pytest.raises(ValueError, match="native"):
            parse_multi_reference(dict(base, native=bad))


def _config(native=True, **over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": [12, 14], "sliding_window": [12, 14]}, "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}},
           "multi_reference": {"directions": ["first", "middle", "last"]}}
    if native is not None:
        cfg["multi_reference"]["native"] = native
    cfg.update(over)
    return cfg


def test_solver_constructs_and_refuses_what_is_outside_the_family(lib):
    import event_based_bos_amd as ebos
    from event_based_bos_amd.solver import WindowPipeline

    make = ebos.solver.collections["contrast_maximization"]
    slv = make((37, 70), (37, 70), solver_config=_config())
    assert slv.multi_reference == {"directions": ["first", "middle", "last"], "normalize": False, "fused": None, "native": True}
    assert slv.fused_loop is False and slv.use_graph is False and slv.resident is False and slv.plan_tile() == (64, 64)
    make((37, 70), (37, 70), solver_config=_config(optimizer={"method": "L-BFGS-B", "n_iter": 5}))
    make((37, 70), (37, 70), solver_config=_config(tile=[32, 32], halo=8, cost_with_weight={"image_variance": 1.0, "flow_norm": 0.1,
                                                                                            "image_gradient": 0.1}))
    refused = (({"cost_with_weight": {"image_variance": 1.0, "gradient_magnitude": 0.5}}, "cost_with_weight.*gradient_magnitude"),
               ({"cost": "gradient_magnitude"}, "gradient_magnitude"),
               ({"iwe": {"blur_sigma": 1}}, "iwe.blur_sigma"),
               ({"outer_padding": 2}, "outer_padding"),
               ({"tile": [45, 80]}, "tile / halo"),
               ({"tile": [32, 32], "halo": 16}, "tile / halo"),
               ({"optimizer": {"method": "grid", "n_iter": 5}}, "optimizer.method"))
    for over, key in refused:
        with pytest.raises(NotImplementedError, match=key) as e:
            make((37, 70), (37, 70), solver_config=_config(**over))
        assert "multi_reference.native" in str(e.value)
        make((37, 70), (37, 70), solver_config=_config(native=False, **over))              # the autograd loop takes every one of them
    # what the block refuses with or without the key
    with pytest.raises(NotImplementedError, match="time_aware"):
        make((37, 70), (37, 70), solver_config=_config(time_aware={"time_bin": 5}))
    for model in ("2d-translation", "rigid-optical-flow"):
        with pytest.raises(NotImplementedError, match="motion_model"):
            make((37, 70), (37, 70), solver_config=_config(motion_model=model))
    with pytest.raises(NotImplementedError, match="multi_reference"):
        WindowPipeline(slv)
    with pytest.raises(ValueError, match="native"):
        make((37, 70), (37, 70), solver_config=_config(native="yes"))
    # without the key the solver's attributes are what they were
    old = make((37, 70), (37, 70), solver_config=_config(native=None))
    assert old.multi_reference == {"directions": ["first", "middle", "last"], "normalize": False, "fused": None}
    assert old.fused_loop is False and old.use_graph is False and old.resident is False and old.plan_tile() == (64, 64)


def test_shipped_native_configuration_constructs(lib):
    """configs/cmax_multi_reference_native.yaml is inside the native family: the solver takes its ``solver`` block as it stands."""
    yaml = pytest.importorskip("yaml")
    import event_based_bos_amd as ebos

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cmax_multi_reference_native.yaml")))
    shape = (cfg["data"]["height"], cfg["data"]["width"])
    slv = ebos.solver.collections[cfg["solver"]["method"]](shape, shape, solver_config=cfg["solver"])
    assert slv.multi_reference["native"] is True and slv.multi_reference["normalize"] is True
    assert (tuple(slv.plan_tile()) + (slv.halo,)) in ebos._hip.slab_multiref_configs()


def _cpu_plan(n=12, tile=(32, 32), shape=(37, 70), fraction=0.0, normalized=True, binned=True):
    """An ``EventPlan`` of CPU tensors (tests/test_multiref.py): the operators' refusals come before any launch."""
    from event_based_bos_amd.event_plan import EventPlan

    n_keys = -(-shape[0] // tile[0]) * -(-shape[1] // tile[1]) * tile[0] * tile[1]
    ko = torch.clamp(torch.arange(n_keys + 1, dtype=torch.int32), max=n) if binned else None
    f = lambda: torch.arange(n, dtype=torch.float32)  # noqa: E731
    return EventPlan(f(), f(), f(), f(), shape, n, n, tile if binned else None, ko, None, dt_bound=1.0, ref_fraction=fraction,
                     normalized_t=normalized)


def test_slab_route_refuses_before_any_launch(lib):
    from event_based_bos_amd import event_plan as EP
    from event_based_bos_amd.solver.multi_reference_loop import MultiReferencePatchLoop

    flow = torch.zeros((2, 37, 70))
    theta = torch.zeros((2, 4, 5))
    ops = [lambda pl, d, **kw: pl.iwe_dense_multi(flow, d, fused="slab", **kw),
           lambda pl, d, **kw: pl.contrast_dense_multi(flow, d, fused="slab", **kw),
           lambda pl, d, **kw: pl.variance_multi_value_and_grad(flow, d, **kw),
           lambda pl, d, **kw: MultiReferencePatchLoop(pl, (12, 14), (12, 14), theta, d, **kw)]
    for op in ops:
        for bad in ([], ["first"] * 5, ["first", "random"], "first"):
            with pytest.raises(ValueError):
                op(_cpu_plan(), bad)
        with pytest.raises(ValueError, match="normalised time"):
            op(_cpu_plan(normalized=False), ["first", "last"])
        with pytest.raises(ValueError, match="reference fraction"):
            op(_cpu_plan(fraction=None), ["first", "last"])
        with pytest.raises(NotImplementedError, match="binned"):
            op(_cpu_plan(binned=False), ["first", "last"])
        deferred = _cpu_plan()
        deferred.__dict__["_deferred"] = True
        with pytest.raises(NotImplementedError, match="deferred=True"):
            op(deferred, ["first", "last"])
        lean = _cpu_plan()
        lean.x = lean.y = lean.dt = lean.p = None
        lean.cpix = torch.zeros(4, dtype=torch.int16)
        with pytest.raises(NotImplementedError, match="lean plan"):
            op(lean, ["first", "last"])
        # an unbuilt (tile, halo): the message names the built ones
        for plan, halo in ((_cpu_plan(tile=(48, 48)), 32), (_cpu_plan(), 16), (_cpu_plan(tile=(45, 80)), "auto")):
            with pytest.raises(NotImplementedError, match=r"\(32, 32, 8\).*\(64, 64, 16\)"):
                op(plan, ["first", "last"], halo=halo)
    # the routes: the halo asked for where it is built, the tile's default built halo for "auto"; True / False / None resolve as before
    job = EP._multiref_job(_cpu_plan(), ["first", "middle", "last"], (2, 2), 8, 3, "slab", "t")
    assert job.fused == "slab" and job.halo == 8 and job.pad == (2, 2) and job.splits == 3 and job.shifts == (0.0, -0.5, -1.0)
    assert EP._multiref_job(_cpu_plan(), ["first"], (0, 0), "auto", None, "slab", "t").halo == 32
    assert EP._multiref_job(_cpu_plan(tile=(64, 64)), ["first"], (0, 0), 16, None, "slab", "t").halo == 16
    assert EP.MULTIREF_DEFAULT_FUSED is False
    assert EP._multiref_job(_cpu_plan(), ["first", "last"], (0, 0), 32, None, None, "t").fused is False
    assert EP._multiref_job(_cpu_plan(), ["first", "last"], (0, 0), 32, None, True, "t").fused is True
    with pytest.raises(ValueError, match="fused"):
        _cpu_plan().iwe_dense_multi(flow, ["first", "last"], fused="slabs")
