"""Launch helpers of the GPU tests of the time-aware kernels (tests/test_gpu_voxel_loop_batch.py, tests/test_gpu_voxel_multiref.py,
tests/test_gpu_voxel_tiles.py): the C entry points on guarded buffers, and stacks of plans.  The image shape, the number of bins and the
plan tile default to the 37 x 70, T = 5, (32, 32) of tests/_voxel_loop_cases.py."""
import ctypes

import numpy as np
import torch

import _voxel_loop_cases as C
from _voxel_loop_cases import H, T5, TILE, W

GUARD = 4096


def P(t):
    return None if t is None else t.data_ptr()


def S():
    from event_based_bos_amd._hip import stream_ptr

    return stream_ptr()


def ok(rc, lib):
    assert rc == 0, lib.ebos_last_error()


def guarded(values=None, shape=None, fill=float("nan")):
    """(whole buffer, the view in its middle): GUARD cells of ``fill`` in front and behind; the middle holds ``values`` (or ``fill``)."""
    shape = tuple(values.shape) if values is not None else tuple(shape)
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device=C.dev())
    view = buf[GUARD:GUARD + n].view(*shape)
    if values is not None:
        view.copy_(values)
    return buf, view


def guards_untouched(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def all_ones(shape):
    """An output whose every byte is 0xFF (every float a NaN): a cell that is not written shows."""
    out = torch.empty(tuple(shape), dtype=torch.float32, device=C.dev())
    out.view(torch.uint8).fill_(0xFF)
    return out


# ---------------------------------------------------------------------------------------------- stacks of plans
def stack_of(ebos, windows, T=T5, tile=TILE, shape=(H, W)):
    plans = [C.plan_of(ebos, ev, tile=tile, T=T, shape=shape) for ev in windows]
    return plans, ebos.EventPlan.stack_time_aware(plans)


class StackWithEmpty(object):
    """The stacked plan of ``plans`` with a window of no events wherever ``plans`` holds None: an empty window's row of the offsets is
    constant, its base, and its n is 0."""

    def __init__(self, ebos, plans):
        live = [p for p in plans if p is not None]
        st = ebos.EventPlan.stack_time_aware(live)
        self.x, self.y, self.dt, self.bins, self.tile = st.x, st.y, st.dt, st.bins, st.tile
        rows, self.ns, at, i = [], [], 0, 0
        for p in plans:
            if p is None:
                rows.append(torch.full_like(st.key_offsets[0], at))
                self.ns.append(0)
            else:
                rows.append(st.key_offsets[i])
                self.ns.append(st.ns[i])
                at += st.ns[i]
                i += 1
        self.key_offsets = torch.stack(rows).contiguous()

    def ns_array(self):
        return (ctypes.c_int64 * len(self.ns))(*self.ns)

    def __len__(self):
        return len(self.ns)


# ---------------------------------------------------------------------------------------------- one reference time
def tiled_batch(lib, stack, voxels, halo, out, pad=0, splits=1, T=T5, shape=(H, W)):
    ok(lib.ebos_iwe_voxel_tiled_batch_f32(P(stack.x), P(stack.y), P(stack.dt), P(stack.bins), P(stack.key_offsets), stack.ns_array(), len(stack),
                                          P(voxels), T, shape[0], shape[1], stack.tile[0], stack.tile[1], halo, splits, pad, pad, P(out), S()),
       lib)


def owner_batch(lib, stack, voxels, g_images, affine, T, pad, g_lo, out, shape=(H, W)):
    ok(lib.ebos_iwe_voxel_owner_bwd_batch_f32(P(stack.x), P(stack.y), P(stack.dt), P(stack.bins), P(stack.key_offsets), stack.ns_array(),
                                              len(stack), P(voxels), T, shape[0], shape[1], stack.tile[0], stack.tile[1], pad, pad,
                                              P(g_images), P(affine), g_lo, P(out), S()), lib)


def owner_single(lib, plan, voxel, g_image, affine, g_lo, pad, shape=(H, W)):
    """The single-window C entry of the one-reference owner backward into a d_voxel whose every byte is 0xFF."""
    T = voxel.shape[0]
    out = all_ones((T, 2) + tuple(shape))
    ok(lib.ebos_iwe_voxel_owner_bwd_f32(P(plan.x), P(plan.y), P(plan.dt), None, P(plan.bins), P(plan.key_offsets), plan.n, P(voxel), T,
                                        shape[0], shape[1], plan.tile[0], plan.tile[1], pad, pad, P(g_image), P(affine), g_lo, P(out), S()),
       lib)
    return out


# ---------------------------------------------------------------------------------------------- K reference times
def c_shifts(plan, directions):
    from event_based_bos_amd.event_plan import multi_reference_shifts

    sh = multi_reference_shifts(plan, directions)
    return (ctypes.c_float * len(sh))(*sh), len(sh)


def forward(lib, plan, voxel, directions, halo, pad, splits=1, shape=(H, W)):
    """The single-window C entry on a NaN-guarded voxel and a zero-filled output between NaN guard cells."""
    T = voxel.shape[0]
    sh, K = c_shifts(plan, directions)
    vbuf, vox = guarded(values=voxel)
    obuf, iwes = guarded(shape=(K, shape[0] + 2 * pad, shape[1] + 2 * pad))
    iwes.zero_()                                                   # (the entry point accumulates: the caller zero-fills once)
    ok(lib.ebos_iwe_voxel_multiref_tiled_f32(P(plan.x), P(plan.y), P(plan.dt), P(plan.bins), P(plan.key_offsets), plan.n, P(vox), T,
                                             shape[0], shape[1], plan.tile[0], plan.tile[1], halo, splits, pad, pad, sh, K, P(iwes), S()),
       lib)
    torch.cuda.synchronize()
    assert guards_untouched(obuf) and guards_untouched(vbuf) and bool(torch.isfinite(iwes).all())
    return iwes


def forward_batch(lib, stack, plan, voxels, directions, halo, pad, splits=1, shape=(H, W)):
    """The batch C entry: voxels [B, T, 2, H, W] -> iwes [B, K, h, w] between NaN guard cells (``plan``: any plan of the stack, for
    the shifts)."""
    B, T = voxels.shape[:2]
    sh, K = c_shifts(plan, directions)
    vbuf, vox = guarded(values=voxels)
    obuf, iwes = guarded(shape=(B, K, shape[0] + 2 * pad, shape[1] + 2 * pad))
    iwes.zero_()
    ok(lib.ebos_iwe_voxel_multiref_tiled_batch_f32(P(stack.x), P(stack.y), P(stack.dt), P(stack.bins), P(stack.key_offsets), stack.ns_array(),
                                                   B, P(vox), T, shape[0], shape[1], stack.tile[0], stack.tile[1], halo, splits, pad, pad, sh, K,
                                                   P(iwes), S()), lib)
    torch.cuda.synchronize()
    assert guards_untouched(obuf) and guards_untouched(vbuf) and bool(torch.isfinite(iwes).all())
    return iwes


def owner_backward(lib, plan, voxel, directions, g_images, affine, g_lo, pad, shape=(H, W)):
    """The single-window C entry into a d_voxel whose every byte is 0xFF (every float a NaN: a cell that is not written shows)."""
    T = voxel.shape[0]
    sh, K = c_shifts(plan, directions)
    out = all_ones((T, 2) + tuple(shape))
    ok(lib.ebos_iwe_voxel_multiref_owner_bwd_f32(P(plan.x), P(plan.y), P(plan.dt), P(plan.bins), P(plan.key_offsets), plan.n, P(voxel), T,
                                                 shape[0], shape[1], plan.tile[0], plan.tile[1], pad, pad, sh, K, P(g_images), P(affine), g_lo,
                                                 P(out), S()), lib)
    return out
