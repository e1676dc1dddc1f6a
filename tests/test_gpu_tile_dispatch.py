"""GPU sweep of the entries that pick a kernel by its (tile_h, tile_w, halo) at run time (csrc/tile_configs.h) and that no other file
drives through every built triple: ``ebos_iwe_dense_tiled_f32`` and ``ebos_iwe_dense_multiref_tiled_f32`` over ``tiled_configs()``,
``ebos_iwe_dense_tiled_multiref_bwd_f32`` over ``slab_multiref_configs()``.  A triple handed to the wrong instantiation (tile height
and width swapped at 16 x 64 or 32 x 64, another halo) bins events of one tile into another's window and fails here.

One 70 x 135 window (tiles overhang both axes on every shape; 64 x 64 makes 2 x 3 of them), 6 000 events on [0, 1], a flow of +-6 px
with one pixel in five between 9 and 100 px so that every halo from 8 to 64 has events whose warp leaves it.  Yardstick: the general
kernel ``ebos_iwe_dense_f32`` on the same float32 inputs, once per reference (dt + shift_k), shared by all triples; the gradient's is
the loop route, ``ebos_iwe_dense_bwd_f32`` per reference.  Bars: those of tests/test_gpu_multiref.py, IWE relative L2 < 1e-4 and
gradient relative L2 < 1e-3 (fused against loop)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _multiref_cases import FML, G, dev, rel  # noqa: E402
from oracle import ebos_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, N, PAD = 70, 135, 6000, 2
SHIFTS = (0.0, -0.25, -0.5, -1.0)   # a 'first' plan's shifts to first, 0.25, middle, last
TILED = ((64, 64, 32), (32, 64, 32), (32, 32, 32), (64, 64, 16), (32, 32, 16), (32, 32, 8), (64, 64, 64), (32, 64, 48), (16, 64, 32))
MULTIREF_SLAB = ((32, 32, 8), (32, 32, 32), (64, 64, 16), (64, 64, 32))
_cache = {}


def built(reader, known):
    """The library's own table where it is there to ask (collection must not need it), else the triples it is known to hold."""
    from event_based_bos_amd import _hip

    return tuple(getattr(_hip, reader)()) if os.path.exists(os.environ.get("EBOS_HIP_LIBRARY", _hip.LIB_PATH)) else known


def tid(t):
    return "x".join(str(int(a)) for a in t)


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def window():
    """(events [N, 4] float64, flow [2, H, W] float64)."""
    if "window" not in _cache:
        ev = O.synth_events(N, H, W, seed=47, tmin=0.0, tmax=1.0)
        ev[0, 2], ev[-1, 2] = 0.0, 1.0
        rs = np.random.RandomState(29)
        flow = rs.uniform(-6.0, 6.0, (2, H, W))
        far = rs.uniform(0.0, 1.0, (2, H, W)) < 0.2
        flow[far] = (rs.uniform(9.0, 100.0, (2, H, W)) * rs.choice([-1.0, 1.0], (2, H, W)))[far]
        _cache["window"] = (ev, flow)
    return _cache["window"]


def plan_of(ebos, tile):
    if ("plan", tile) not in _cache:
        _cache["plan", tile] = ebos.EventPlan.build(G(window()[0]), (H, W), "first", True, tile=tile, emit="full")
    return _cache["plan", tile]


def general_iwe(ebos, shift):
    """[H + 2 PAD, W + 2 PAD] of the general kernel with dt + shift: made once, read by every triple."""
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    if ("general", shift) not in _cache:
        plan, flow32 = plan_of(ebos, (32, 32)), G(window()[1], torch.float32)
        dt = plan.dt if shift == 0.0 else (plan.dt + shift).contiguous()
        out = torch.zeros((H + 2 * PAD, W + 2 * PAD), dtype=torch.float32, device=dev())
        check(ebos.load_library().ebos_iwe_dense_f32(ptr(plan.x), ptr(plan.y), ptr(dt), None, plan.n, ptr(flow32), H, W, W, PAD, PAD, ptr(out),
                                                     stream_ptr()), "ebos_iwe_dense")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and float(out.sum()) > 0.3 * N
        _cache["general", shift] = out
    return _cache["general", shift]


def test_the_sweeps_are_the_built_sets(ebos):
    from event_based_bos_amd import _hip

    assert set(built("tiled_configs", TILED)) == set(_hip.tiled_configs()) == set(TILED)
    assert set(built("slab_multiref_configs", MULTIREF_SLAB)) == set(_hip.slab_multiref_configs()) == set(MULTIREF_SLAB)
    ev, flow = window()
    moved = np.abs(ev[:, 2:3] * flow[:, ev[:, 0].astype(int), ev[:, 1].astype(int)].T).max(1)   # px, at shift 0 (|dt + shift_k| <= 1 too)
    for halo in sorted({t[2] for t in TILED}):
        assert int((moved > halo + 1).sum()) > 20, halo                                    # every halo has events whose taps leave it


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("triple", built("tiled_configs", TILED), ids=tid)
def test_dense_tiled_entries_are_the_general_kernel(ebos, triple, splits):
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    lib = ebos.load_library()
    th, tw, hl = triple
    plan, flow32 = plan_of(ebos, (th, tw)), G(window()[1], torch.float32)
    shape = (H + 2 * PAD, W + 2 * PAD)
    got = torch.zeros(shape, dtype=torch.float32, device=dev())
    check(lib.ebos_iwe_dense_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), None, ptr(plan.key_offsets), plan.n, ptr(flow32), H, W, th, tw,
                                       hl, splits, PAD, PAD, ptr(got), stream_ptr()), "ebos_iwe_dense_tiled")
    err = rel(got, general_iwe(ebos, 0.0))
    print(f"TD|single|{tid(triple)}|splits {splits}|{err:.3e}")
    assert bool(torch.isfinite(got).all()) and err < 1e-4, (triple, splits, err)
    # K references per pass: one, and as many as the triple's LDS windows allow
    k_max = max(K for K in (1, 2, 3, 4) if lib.ebos_iwe_multiref_fits(th, tw, hl, K) != 0)
    for K in sorted({1, k_max}):
        iwes = torch.zeros((K,) + shape, dtype=torch.float32, device=dev())
        shifts = (ctypes.c_float * K)(*SHIFTS[:K])
        check(lib.ebos_iwe_dense_multiref_tiled_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32), H, W,
                                                    th, tw, hl, splits, PAD, PAD, shifts, K, ptr(iwes), stream_ptr()),
              "ebos_iwe_dense_multiref_tiled")
        errs = [rel(iwes[k], general_iwe(ebos, SHIFTS[k])) for k in range(K)]
        print(f"TD|multiref|{tid(triple)}|splits {splits}|K {K}|{max(errs):.3e}")
        assert bool(torch.isfinite(iwes).all()) and max(errs) < 1e-4, (triple, splits, K, errs)


@pytest.mark.parametrize("triple", built("slab_multiref_configs", MULTIREF_SLAB), ids=tid)
def test_multiref_slab_backward_is_the_loop_route(ebos, triple):
    from event_based_bos_amd import event_plan as EP

    th, tw, hl = triple
    plan, flow32 = plan_of(ebos, (th, tw)), G(window()[1], torch.float32)
    job = EP._multiref_job(plan, list(FML), (PAD, PAD), hl, 2, "slab", "test")
    assert job.route == "slab" and job.halo == hl
    iwes, _, _ = EP._launch_multiref_slab_fwd(plan, flow32, job, 0, False)
    errs = [rel(iwes[k], general_iwe(ebos, s)) for k, s in enumerate(job.shifts)]
    affine = torch.tensor([[0.37, -0.11], [0.21, 0.05], [-0.4, 0.3]], dtype=torch.float32, device=dev())
    got = EP._launch_multiref_slab_bwd(plan, flow32, job, iwes, affine, 0)
    loop = EP._launch_multiref_bwd(plan, flow32, EP._multiref_job(plan, list(FML), (PAD, PAD), 32, None, False, "test"), iwes, affine, 0)
    print(f"TD|slab|{tid(triple)}|iwe {max(errs):.3e}|d_flow {rel(got, loop):.3e}")
    assert job.shifts == (0.0, -0.5, -1.0) and max(errs) < 1e-4
    assert bool(torch.isfinite(got).all()) and int(torch.count_nonzero(got)) > 0 and rel(got, loop) < 1e-3
