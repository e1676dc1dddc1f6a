"""CPU checks of the batched time-aware loop's boundary: the layout of ``ebos_cmax_voxel_batch_problem`` against its ctypes mirror, the
argument validation of ``ebos_cmax_voxel_solve_batch_f32`` (before any HIP call: usable without a GPU), what
``EventPlan.stack_time_aware`` refuses, and ``ContrastMaximization.estimate_batch`` outside the native family."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


def test_batch_problem_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """``ebos_cmax_voxel_batch_problem`` as a C compiler lays it out == ``_hip.CmaxVoxelBatchProblem`` (size and every field offset),
    by the gcc ``offsetof`` method of tests/test_abi.py; ``n`` is an array of EBOS_CMAX_VOXEL_MAX_BATCH int64."""
    from event_based_bos_amd import _hip

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    c_name, mirror = "ebos_cmax_voxel_batch_problem", _hip.CmaxVoxelBatchProblem
    fields = [f[0] for f in mirror._fields_]
    hdr = open(os.path.join(ROOT, "include", "ebos_hip.h")).read()
    assert "#define EBOS_CMAX_VOXEL_MAX_BATCH %d\n" % _hip.CMAX_VOXEL_MAX_BATCH in hdr
    body = hdr[hdr.index("typedef struct %s {" % c_name):hdr.index("} %s;" % c_name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split("{", 1)[1].split(";"):
        declared += re.findall(r"[*\s,]([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[A-Za-z0-9_]+\])?\s*(?=,|$)", stmt.strip())
    assert declared == fields, (declared, fields)
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ebos_hip.h"', 'int main(void) {',
             '  printf("%%zu\\n", sizeof(%s));' % c_name, '  printf("%%zu\\n", sizeof(((%s*)0)->n));' % c_name]
    lines += [f'  printf("%zu\\n", offsetof({c_name}, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(mirror), 8 * _hip.CMAX_VOXEL_MAX_BATCH] + [getattr(mirror, f).offset for f in fields]
    # the single problem is not grown: the batch problem is the single one's fields behind B, the streams and the counts
    assert [f[0] for f in _hip.CmaxVoxelProblem._fields_[6:]] == fields[7:]


def _problem(B=3):
    """A problem whose pointers are non-NULL dummies: validation never dereferences them, and a valid one would need a GPU."""
    from event_based_bos_amd import _hip

    q = _hip.CmaxVoxelBatchProblem()
    for name, kind in q._fields_:
        if kind is _hip._P:
            setattr(q, name, 0x1000)
    q.B = B
    for b in range(min(B, _hip.CMAX_VOXEL_MAX_BATCH)):
        q.n[b] = 100 * b                                   # (the first window is empty: valid)
    q.H, q.W, q.tile_h, q.tile_w, q.halo, q.splits = 37, 70, 32, 32, 32, 1
    q.T, q.scheme, q.t0_index, q.route, q.owner_bwd = 5, _hip.FLOW_UPWIND, 2, _hip.FLOW_ROUTE_AUTO, 1
    q.gh, q.gw, q.patch_h, q.patch_w, q.slide_h, q.slide_w = 4, 5, 12, 14, 12, 14
    q.w_variance, q.lr, q.beta1, q.beta2, q.eps = 1.0, 0.05, 0.9, 0.999, 1e-8
    q.cost_scratch_bytes, q.adjoint_workspace_elems, q.losses_cap = 1 << 24, 1 << 30, 8
    return q


def test_batch_solve_validates_before_any_launch(lib):
    from event_based_bos_amd import _hip

    def refused(q, n_iter, word, rc=-1):
        got = lib.ebos_cmax_voxel_solve_batch_f32(None if q is None else ctypes.byref(q), n_iter, None)
        msg = lib.ebos_last_error()
        assert got == rc and word in msg, (got, msg)

    refused(None, 1, b"NULL problem")
    for B in (0, 65):
        refused(_problem(B), 1, b"B = %d is outside [1, 64]" % B)
    for T in (0, 256):
        q = _problem()
        q.T = T
        refused(q, 1, b"outside [1, 255]")
    q = _problem()
    q.scheme = _hip.FLOW_SAME                             # a scheme of the voxel, not of this loop
    refused(q, 1, b"scheme 2")
    for name, word in (("theta", b"NULL theta"), ("exp_avg_sq", b"NULL theta"), ("key_offsets", b"NULL plan buffer"),
                       ("bins", b"NULL plan buffer"), ("voxel", b"NULL image"), ("iwe", b"NULL image"), ("affine", b"NULL image"),
                       ("reg_partials", b"NULL image")):
        q = _problem()
        setattr(q, name, None)
        refused(q, 1, word)
    q = _problem()
    q.has_clamp, q.voxel_clamped = 1, None
    refused(q, 1, b"has_clamp")
    q = _problem()
    q.w_image_gradient, q.d_reg = 0.1, None
    refused(q, 1, b"d_reg")
    q = _problem()
    q.n[1] = -1
    refused(q, 1, b"window 1 has n = -1")
    q = _problem()
    q.n[1], q.n[2] = 2 ** 31 - 1, 1
    refused(q, 1, b"INT32_MAX")
    # the scratch of the variance is the one of B images, not of one
    q = _problem()
    one, three = lib.ebos_cost_scratch_bytes(1), lib.ebos_cost_scratch_bytes(3)
    assert three > one
    q.cost_scratch_bytes = three - 1
    refused(q, 1, b"cost_scratch too small for 3 windows", rc=-4)           # EBOS_ERR_SCRATCH
    # the workspace the adjoint of B voxels reports
    q = _problem()
    q.route = _hip.FLOW_ROUTE_STEPS
    need1 = lib.ebos_flow_voxel_advect_adjoint_workspace(q.scheme, 1, q.T, q.H, q.W, q.t0_index, 0, q.route)
    need3 = lib.ebos_flow_voxel_advect_adjoint_workspace(q.scheme, 3, q.T, q.H, q.W, q.t0_index, 0, q.route)
    assert need3 > need1 > 0
    q.adjoint_workspace_elems = need1                      # enough for one window, short for three
    refused(q, 1, b"adjoint_workspace", rc=-4)
    refused(_problem(), -1, b"negative n_iter")
    # the gradient entry shares the checks
    assert lib.ebos_cmax_voxel_gradient_batch_f32(None, None) == -1 and b"NULL problem" in lib.ebos_last_error()
    q = _problem(65)
    assert lib.ebos_cmax_voxel_gradient_batch_f32(ctypes.byref(q), None) == -1 and b"B = 65" in lib.ebos_last_error()


def test_batched_stages_validate_before_any_launch(lib):
    p, ns = 0x1000, (ctypes.c_int64 * 3)(10, 0, 20)
    assert lib.ebos_upsample_patch_flow_batch_f32(p, 0, 4, 5, 12, 14, 12, 14, 37, 70, p, None) == -1 and b"B = 0" in lib.ebos_last_error()
    assert lib.ebos_upsample_patch_flow_batch_f32(None, 3, 4, 5, 12, 14, 12, 14, 37, 70, p, None) == -1
    assert lib.ebos_flow_regularisers_batch_f32(p, 65, 37, 70, 0.1, 0.1, p, p, None) == -1 and b"B = 65" in lib.ebos_last_error()
    assert lib.ebos_flow_regularisers_batch_f32(p, 3, 37, 70, 0.1, 0.1, p, None, None) == -1
    tiled = lambda **o: lib.ebos_iwe_voxel_tiled_batch_f32(*dict(dict(xs=p, ys=p, dts=p, bins=p, ko=p, ns=ns, B=3, voxel=p, T=5, H=37, W=70,  # noqa: E731
                                                                      th=32, tw=32, halo=32, splits=1, ph=0, pw=0, iwe=p, s=None), **o).values())
    assert tiled(B=0) == -1 and tiled(T=256) == -1 and b"outside [1, 255]" in lib.ebos_last_error()
    assert tiled(ko=None) == -1 and tiled(ns=None) == -1 and tiled(bins=None) == -1 and tiled(splits=0) == -1
    bad = (ctypes.c_int64 * 3)(10, -2, 20)
    assert tiled(ns=bad) == -1 and b"window 1" in lib.ebos_last_error()
    owner = lambda **o: lib.ebos_iwe_voxel_owner_bwd_batch_f32(*dict(dict(xs=p, ys=p, dts=p, bins=p, ko=p, ns=ns, B=3, voxel=p, T=5, H=37,  # noqa: E731
                                                                          W=70, th=32, tw=32, ph=0, pw=0, g=p, affine=None, g_lo=0, dv=p,
                                                                          s=None), **o).values())
    assert owner(B=65) == -1 and owner(T=0) == -1 and owner(ko=None) == -1 and b"key_offsets" in lib.ebos_last_error()
    assert owner(dv=None) == -1 and owner(th=0) == -1 and owner(ns=bad) == -1 and owner(xs=None) == -1
    adam = lambda **o: lib.ebos_upsample_patch_flow_bwd_adam_batch_f32(*dict(dict(dd=p, B=3, gh=4, gw=5, ph=12, pw=14, sh=12, sw=14, H=37,  # noqa: E731
                                                                                W=70, scratch=p, dg=p, theta=p, m=p, v=p, lr=0.05, b1=0.9,
                                                                                b2=0.999, eps=1e-8, t=1, step=p, contrast=p, scale=-1.0,
                                                                                reg=None, n_reg=0, losses=p, cap=8, mask=None, s=None),
                                                                           **o).values())
    assert adam(B=0) == -1 and adam(t=0) == -1 and adam(theta=None) == -1 and adam(n_reg=4) == -1 and adam(scratch=None) == -1
    assert lib.ebos_upsample_patch_flow_bwd_batch_f32(p, 3, 4, 5, 12, 14, 12, 14, 37, 70, p, None, None) == -1


def _cpu_plan(n=12, tile=(32, 32), time_bin=5, binned=True, bins=True, shape=(37, 70), dt_bound=1.0):
    """An ``EventPlan`` of CPU tensors: ``stack_time_aware`` checks and concatenates, it launches nothing."""
    from event_based_bos_amd.event_plan import EventPlan

    n_keys = -(-shape[0] // tile[0]) * -(-shape[1] // tile[1]) * tile[0] * tile[1]
    ko = torch.clamp(torch.arange(n_keys + 1, dtype=torch.int32), max=n) if binned else None
    f = lambda: torch.arange(n, dtype=torch.float32)  # noqa: E731
    return EventPlan(f(), f(), f(), f(), shape, n, n, tile if binned else None, ko, None, dt_bound=dt_bound,
                     bins=torch.zeros(n, dtype=torch.uint8) if bins else None, time_bin=time_bin if bins else None)


def test_stack_time_aware_stacks_and_refuses():
    from event_based_bos_amd.event_plan import EventPlan, TimeAwarePlanStack

    a, b, c = _cpu_plan(12), _cpu_plan(0), _cpu_plan(7)
    st = EventPlan.stack_time_aware([a, b, c])
    assert isinstance(st, TimeAwarePlanStack) and len(st) == 3 and st.ns == [12, 0, 7] and st.n == 19 and list(st.ns_array()) == [12, 0, 7]
    assert st.x.shape == (19,) and st.bins.shape == (19,) and st.bins.dtype == torch.uint8
    ko = st.key_offsets
    assert ko.dtype == torch.int32 and ko.shape == (3, a.key_offsets.numel()) and ko.is_contiguous()
    # row b = the window's offsets shifted by its base: window b is the slice ko[b][0] .. ko[b][-1] of the streams
    assert ko[:, 0].tolist() == [0, 12, 12] and ko[:, -1].tolist() == [12, 12, 19]
    assert torch.equal(ko[2] - 12, c.key_offsets) and torch.equal(st.x[12:], c.x)
    with pytest.raises(ValueError, match="tile"):
        EventPlan.stack_time_aware([a, _cpu_plan(tile=(64, 64))])
    with pytest.raises(ValueError, match="time_bin"):
        EventPlan.stack_time_aware([a, _cpu_plan(time_bin=15)])
    with pytest.raises(ValueError, match="un-binned"):
        EventPlan.stack_time_aware([a, _cpu_plan(binned=False)])
    with pytest.raises(ValueError, match="no time bins"):
        EventPlan.stack_time_aware([_cpu_plan(bins=False)])
    with pytest.raises(ValueError, match="image_size"):
        EventPlan.stack_time_aware([a, _cpu_plan(shape=(37, 64))])
    with pytest.raises(ValueError, match="direction"):
        EventPlan.stack_time_aware([a, _cpu_plan(dt_bound=0.5)])
    deferred = _cpu_plan()
    deferred.__dict__["_deferred"] = True
    with pytest.raises(ValueError, match="deferred"):
        EventPlan.stack_time_aware([a, deferred])
    with pytest.raises(ValueError, match="no plans"):
        EventPlan.stack_time_aware([])
    big = _cpu_plan()
    big.n = 2 ** 31 - 5                                   # (validation reads the counts before it touches the streams)
    with pytest.raises(ValueError, match="INT32_MAX"):
        EventPlan.stack_time_aware([big, a])


def test_stack_of_one_plan_shares_the_plans_storage():
    """One window is a batch of one without a copy: the stack's streams are views of the plan's, its offsets the plan's own with a
    leading dimension (the base is 0).  Two plans still concatenate."""
    from event_based_bos_amd.event_plan import EventPlan

    a = _cpu_plan(12)
    st = EventPlan.stack_time_aware([a])
    assert len(st) == 1 and st.ns == [a.n] == [12] and st.n == 12 and list(st.ns_array()) == [12]
    for k in ("x", "y", "dt", "bins"):
        assert getattr(st, k).data_ptr() == getattr(a, k).data_ptr() and getattr(st, k).shape == (12,), k
    assert st.key_offsets.data_ptr() == a.key_offsets.data_ptr() and st.key_offsets.dtype == torch.int32
    assert st.key_offsets.shape == (1, a.key_offsets.numel()) and st.key_offsets.is_contiguous() and torch.equal(st.key_offsets[0], a.key_offsets)
    # a plan whose streams are longer than n (a build pads them): the view stops at n
    padded = _cpu_plan(12)
    padded.n = 9
    st = EventPlan.stack_time_aware([padded])
    assert st.x.shape == (9,) and st.bins.shape == (9,) and st.x.data_ptr() == padded.x.data_ptr() and st.ns == [9]
    c = _cpu_plan(7)
    two = EventPlan.stack_time_aware([a, c])
    assert two.x.data_ptr() != a.x.data_ptr() and torch.equal(two.x, torch.cat([a.x, c.x])) and torch.equal(two.bins, torch.cat([a.bins, c.bins]))
    assert two.key_offsets.shape == (2, a.key_offsets.numel()) and torch.equal(two.key_offsets[0], a.key_offsets)
    assert torch.equal(two.key_offsets[1] - 12, c.key_offsets)


def _config(**over):
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0,
           "patch": {"size": [12, 14], "sliding_window": [12, 14]}, "optimizer": {"method": "Adam", "n_iter": 5, "parameters": {"lr": 0.05}},
           "time_aware": {"time_bin": 5, "scheme": "upwind", "t0_location": "middle", "native": True}}
    cfg.update(over)
    return cfg


def test_estimate_batch_outside_the_native_family_is_the_loop_of_estimate(lib):
    import event_based_bos_amd as ebos

    make = ebos.solver.collections["contrast_maximization"]
    no_native = _config()
    no_native["time_aware"] = {"time_bin": 5}
    no_time_aware = _config()
    no_time_aware.pop("time_aware")
    cases = {"scipy": _config(optimizer={"method": "L-BFGS-B", "n_iter": 5}), "no native": no_native, "no time_aware": no_time_aware,
             "2-DoF": dict(no_time_aware, motion_model="2d-translation")}
    for name, cfg in cases.items():
        slv = make((37, 70), (37, 70), solver_config=cfg)
        assert not slv._native_batch(), name
        seen = []

        def estimate(ev, slv=slv, seen=seen):
            seen.append(ev)
            slv.history = [float(len(seen)), -1.0]
            return np.full((2, 37, 70), float(len(seen)))

        slv.estimate = estimate
        windows = [np.zeros((3, 4)), np.ones((5, 4)), np.zeros((0, 4))]
        flows = slv.estimate_batch(windows, max_batch=2)
        assert flows.shape == (3, 2, 37, 70) and flows.dtype == np.float64, name
        assert [f[0, 0, 0] for f in flows] == [1.0, 2.0, 3.0] and all(a is b for a, b in zip(seen, windows)), name
        assert slv.histories == [[1.0, -1.0], [2.0, -1.0], [3.0, -1.0]], name
        assert slv.estimate_batch([]).shape == (0, 2, 37, 70)

        def refuse(ev):
            raise ValueError("this window")

        slv.estimate = refuse                               # a window estimate refuses is refused the same way
        with pytest.raises(ValueError, match="this window"):
            slv.estimate_batch(windows)
    native = make((37, 70), (37, 70), solver_config=_config())
    assert native._native_batch()
    with pytest.raises(ValueError, match="max_batch"):
        native.estimate_batch([np.zeros((3, 4))], max_batch=0)
