"""Shared helpers of tests/test_multiref_loop.py and tests/test_gpu_multiref_loop.py: the raw C calls of the K-image slab pipeline
with guarded outputs, the single form on ``dt + shift_k`` it is compared with bit for bit, and the solver configurations of the
``multi_reference: {native: true}`` block.  Windows, flows and float64 yardsticks come from tests/_multiref_cases.py."""
import ctypes

import torch

import _multiref_cases as C

GUARD = 64            # floats in front of and behind every guarded output
SENTINEL = -12345.5   # what the guard cells hold


def c_floats(values):
    return (ctypes.c_float * len(values))(*values)


def guarded(shape, fill=float("nan"), dtype=torch.float32):
    """(flat storage, view): ``view`` is ``shape`` inside ``storage``, filled with ``fill``, GUARD sentinel cells on either side."""
    n = 1
    for s in shape:
        n *= s
    store = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=C.dev())
    view = store[GUARD:GUARD + n].view(*shape)
    view.fill_(fill)
    return store, view


def guards_intact(store):
    return bool((store[:GUARD] == SENTINEL).all()) and bool((store[-GUARD:] == SENTINEL).all())


def padded_dt(plan, shift):
    """``plan.dt + shift`` in float32 -- the loop route's event times of one reference -- padded for 16-byte loads like the plan's arrays."""
    out = torch.zeros((plan.n + 3) // 4 * 4 + 4, dtype=torch.float32, device=plan.device)
    out[:plan.n] = plan.dt + shift
    return out


def slab_single(lib, plan, dts, flow32, halo, splits, pad, want_variance=0, omit=False):
    """``ebos_iwe_dense_slab_f32`` on the plan's (x, y) arrays with ``dts`` as event times (no compact arrays, unit weights)."""
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    H, W = plan.image_size
    th, tw = plan.tile
    nbytes = int(lib.ebos_iwe_slab_workspace_bytes(H, W, th, tw, halo, splits, pad, pad))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=plan.device)
    iwe = torch.full((H + 2 * pad, W + 2 * pad), float("nan"), dtype=torch.float32, device=plan.device)
    var = torch.empty(1, dtype=torch.float32, device=plan.device) if want_variance else None
    check(lib.ebos_iwe_dense_slab_f32(ptr(plan.x), ptr(plan.y), ptr(dts), None, None, None, None, ptr(plan.key_offsets), plan.n, ptr(flow32),
                                      H, W, th, tw, halo, splits, pad, pad, ptr(ws), nbytes, ptr(iwe), int(want_variance), int(omit), ptr(var),
                                      None, None, stream_ptr()), "ebos_iwe_dense_slab")
    return iwe, var


def slab_multi(lib, plan, shifts, flow32, halo, splits, pad, want_variance=0, omit=False, ws=None):
    """``ebos_iwe_dense_slab_multiref_f32`` into NaN-filled, guarded outputs -> (iwes, variances, moments, their storages, workspace)."""
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    H, W = plan.image_size
    th, tw = plan.tile
    K = len(shifts)
    nbytes = int(lib.ebos_iwe_slab_multiref_workspace_bytes(K, H, W, th, tw, halo, splits, pad, pad))
    assert nbytes > 0
    if ws is None:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=plan.device)
    s_iwes, iwes = guarded((K, H + 2 * pad, W + 2 * pad))
    s_var, var = guarded((K,))
    s_mom, mom = guarded((K, 2), dtype=torch.float64)
    check(lib.ebos_iwe_dense_slab_multiref_f32(ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n, ptr(flow32), H, W, th, tw,
                                               halo, splits, pad, pad, c_floats(shifts), K, ptr(ws), nbytes, ptr(iwes), int(want_variance),
                                               int(omit), ptr(var) if want_variance else None, ptr(mom) if want_variance else None,
                                               stream_ptr()), "ebos_iwe_dense_slab_multiref")
    return iwes, var, mom, (s_iwes, s_var, s_mom), ws


def native_config(directions, n_iter=5, tile=C.TILE, method="Adam", **over):
    """tests/_multiref_cases.solver_config with ``native: true`` in the block."""
    cfg = C.solver_config(directions, n_iter=n_iter, tile=tile, method=method, **over)
    cfg["multi_reference"]["native"] = True
    return cfg
