"""CPU checks of the native time-aware loop's boundary: the ``time_aware.native`` key, the argument validation of
``ebos_cmax_voxel_solve_f32`` and ``ebos_iwe_voxel_owner_bwd_f32`` (before any HIP call: usable without a GPU), the layout of
``ebos_cmax_voxel_problem`` against its ctypes mirror, and what a ``native`` solver refuses at construction."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


def test_parse_time_aware_native_key():
    from event_based_bos_amd.solver.contrast_maximization import parse_time_aware

    assert parse_time_aware({"time_bin": 5, "native": True})["native"] is True
    assert parse_time_aware({"time_bin": 5, "native": False})["native"] is False
    # the default is false: a block without the key parses to what it always did (tests/test_warp_voxel.py compares that dict)
    assert parse_time_aware({"time_bin": 5}).get("native", False) is False
    assert parse_time_aware(None) is None
    with pytest.raises(ValueError):
        parse_time_aware({"time_bin": 5, "natve": True})
    with pytest.raises(ValueError):
        parse_time_aware({"time_bin": 5, "native": "yes"})


def test_default_backward_of_the_loop_follows_the_measurement():
    """the owner kernel where it was measured faster (2 M events, T = 15), the atomic kernel elsewhere."""
    from event_based_bos_amd.solver.time_aware_loop import default_owner_bwd

    assert default_owner_bwd(15, 2_000_000) is True
    assert default_owner_bwd(5, 2_000_000) is False and default_owner_bwd(15, 100_000) is False and default_owner_bwd(5, 100_000) is False


def _problem():
    """A problem whose pointers are non-NULL dummies: validation never dereferences them, and a valid one would need a GPU."""
    from event_based_bos_amd import _hip

    q = _hip.CmaxVoxelProblem()
    for name, kind in q._fields_:
        if kind is _hip._P:
            setattr(q, name, 0x1000)
    q.n, q.H, q.W, q.tile_h, q.tile_w, q.halo, q.splits = 100, 37, 70, 32, 32, 32, 1
    q.T, q.scheme, q.t0_index, q.route, q.owner_bwd = 5, _hip.FLOW_UPWIND, 2, _hip.FLOW_ROUTE_AUTO, 1
    q.gh, q.gw, q.patch_h, q.patch_w, q.slide_h, q.slide_w = 4, 5, 12, 14, 12, 14
    q.w_variance, q.lr, q.beta1, q.beta2, q.eps = 1.0, 0.05, 0.9, 0.999, 1e-8
    q.cost_scratch_bytes, q.adjoint_workspace_elems, q.losses_cap = 1 << 20, 1 << 30, 8
    return q


def test_solve_validates_before_any_launch(lib):
    def refused(q, n_iter, word, rc=-1):
        got = lib.ebos_cmax_voxel_solve_f32(None if q is None else ctypes.byref(q), n_iter, None)
        msg = lib.ebos_last_error()
        assert got == rc and word in msg, (got, msg)

    refused(None, 1, b"NULL problem")
    for T in (0, 256):
        q = _problem()
        q.T = T
        refused(q, 1, b"outside [1, 255]")
    q = _problem()
    q.scheme = 7
    refused(q, 1, b"scheme 7")
    q = _problem()
    q.scheme = 2                                          # EBOS_FLOW_SAME: a scheme of the voxel, not of this loop
    refused(q, 1, b"scheme 2")
    q = _problem()
    q.theta = None
    refused(q, 1, b"NULL theta")
    refused(_problem(), -1, b"negative n_iter")
    q = _problem()
    q.t0_index = 5
    refused(q, 1, b"t0_index")
    q = _problem()
    q.has_clamp, q.voxel_clamped = 1, None
    refused(q, 1, b"has_clamp")
    q = _problem()
    q.w_flow_norm, q.d_reg = 0.1, None
    refused(q, 1, b"d_reg")
    # the workspace the voxel's adjoint reports: the per-step route needs 4 H W floats
    from event_based_bos_amd import _hip
    q = _problem()
    q.route, q.adjoint_workspace_elems = _hip.FLOW_ROUTE_STEPS, 10
    need = lib.ebos_flow_voxel_advect_adjoint_workspace(q.scheme, 1, q.T, q.H, q.W, q.t0_index, 0, q.route)
    assert need == 4 * 37 * 70
    refused(q, 1, b"adjoint_workspace", rc=-4)            # EBOS_ERR_SCRATCH
    # the gradient entry shares the checks
    assert lib.ebos_cmax_voxel_gradient_f32(None, None) == -1 and b"NULL problem" in lib.ebos_last_error()


def test_single_entries_are_adapters_of_the_batch_loop(lib):
    """``ebos_cmax_voxel_solve_f32`` / ``_gradient_f32`` run the batch loop's checks on a batch of one: a refusal names the entry
    point the caller used, the scratch asked for is the one of ONE window, and ``n`` is checked as the window's count."""
    def solve(q):
        return lib.ebos_cmax_voxel_solve_f32(ctypes.byref(q), 1, None), lib.ebos_last_error()

    def gradient(q):
        return lib.ebos_cmax_voxel_gradient_f32(ctypes.byref(q), None), lib.ebos_last_error()

    for call, who in ((solve, b"ebos_cmax_voxel_solve:"), (gradient, b"ebos_cmax_voxel_gradient:")):
        q = _problem()
        q.T = 0
        rc, msg = call(q)
        assert rc == -1 and msg.startswith(who) and b"_batch" not in msg and b"outside [1, 255]" in msg, (rc, msg)
        q = _problem()
        q.cost_scratch_bytes = lib.ebos_cost_scratch_bytes(1)              # exactly enough for one window: past this check
        q.theta = None
        rc, msg = call(q)
        assert rc == -1 and msg.startswith(who) and b"NULL theta" in msg, (rc, msg)
        q = _problem()
        q.cost_scratch_bytes = lib.ebos_cost_scratch_bytes(1) - 1
        rc, msg = call(q)
        assert rc == -4 and msg.startswith(who) and b"_batch" not in msg and b"cost_scratch too small for 1 windows" in msg, (rc, msg)
        q = _problem()
        q.n = -1
        rc, msg = call(q)
        assert rc == -1 and msg.startswith(who) and b"n = -1" in msg, (rc, msg)
        q = _problem()
        q.n = 2 ** 31
        rc, msg = call(q)
        assert rc == -1 and msg.startswith(who) and b"INT32_MAX" in msg, (rc, msg)
    assert lib.ebos_cmax_voxel_solve_f32(None, 1, None) == -1 and lib.ebos_last_error() == b"ebos_cmax_voxel_solve: NULL problem"
    assert lib.ebos_cmax_voxel_gradient_f32(None, None) == -1 and lib.ebos_last_error() == b"ebos_cmax_voxel_gradient: NULL problem"
    # exactly the scratch of one window passes every check: with no iterations asked for, nothing is launched
    q = _problem()
    q.cost_scratch_bytes = lib.ebos_cost_scratch_bytes(1)
    assert lib.ebos_cmax_voxel_solve_f32(ctypes.byref(q), 0, None) == 0


def test_owner_backward_validates_before_any_launch(lib):
    p = 0x1000
    args = dict(xs=p, ys=p, dts=p, weight=None, bins=p, key_offsets=p, n=10, voxel=p, T=5, H=37, W=70, tile_h=32, tile_w=32, pad_h=0,
                pad_w=0, g_image=p, affine=None, g_lo=0, d_voxel=p, stream=None)

    def call(**over):
        a = dict(args, **over)
        return lib.ebos_iwe_voxel_owner_bwd_f32(*a.values())

    assert call(key_offsets=None) == -1 and b"key_offsets is NULL" in lib.ebos_last_error()
    assert call(T=0) == -1 and b"outside [1, 255]" in lib.ebos_last_error()
    assert call(T=256) == -1
    assert call(d_voxel=None) == -1 and call(tile_h=0) == -1 and call(bins=None) == -1


def test_voxel_problem_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """``ebos_cmax_voxel_problem`` as a C compiler lays it out == ``_hip.CmaxVoxelProblem`` (size and every field offset), by the
    method of tests/test_abi.py::test_problem_struct_layout_matches_the_ctypes_mirror."""
    from event_based_bos_amd import _hip

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    c_name, mirror = "ebos_cmax_voxel_problem", _hip.CmaxVoxelProblem
    fields = [f[0] for f in mirror._fields_]
    hdr = open(os.path.join(ROOT, "include", "ebos_hip.h")).read()
    body = hdr[hdr.index("typedef struct %s {" % c_name):hdr.index("} %s;" % c_name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
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
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]


def _config(**over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": [12, 14], "sliding_window": [12, 14]}, "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}},
           "time_aware": {"time_bin": 5, "scheme": "upwind", "t0_location": "middle", "native": True}}
    cfg.update(over)
    return cfg


def test_native_solver_refuses_what_is_outside_its_family(lib):
    import event_based_bos_amd as ebos

    make = ebos.solver.collections["contrast_maximization"]
    slv = make((37, 70), (37, 70), solver_config=_config())
    assert slv.time_aware["native"] is True and slv.plan_tile() == (64, 64)          # a built tile of the time-aware forward kernel
    assert make((37, 70), (37, 70), solver_config=_config(tile=[32, 32])).plan_tile() == (32, 32)
    assert make((37, 70), (37, 70), solver_config=_config(halo=8)).plan_tile() == (32, 32)    # the one tile built with halo 8
    make((37, 70), (37, 70), solver_config=_config(cost_with_weight={"image_variance": 1.0, "flow_norm": 0.1, "image_gradient": 0.1}))
    make((37, 70), (37, 70), solver_config=_config(optimizer={"method": "L-BFGS-B", "n_iter": 5}))
    with pytest.raises(NotImplementedError, match="blur_sigma"):
        make((37, 70), (37, 70), solver_config=_config(iwe={"blur_sigma": 1}))
    with pytest.raises(NotImplementedError, match="cost"):
        make((37, 70), (37, 70), solver_config=_config(cost="gradient_magnitude"))
    with pytest.raises(NotImplementedError, match="optimizer.method"):
        make((37, 70), (37, 70), solver_config=_config(optimizer={"method": "grid", "n_iter": 5}))
    # without the key the same configurations are the autograd loop's, as before
    off = _config(iwe={"blur_sigma": 1})
    off["time_aware"].pop("native")
    slv = make((37, 70), (37, 70), solver_config=off)
    assert slv.time_aware.get("native", False) is False and slv.plan_tile() != (64, 64)
