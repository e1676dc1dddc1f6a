"""Poisson integration of BOS flows on the GPU (reference: src/utils/stat_utils.py:142-199, ``poisson_reconstruct``, and
src/visualizer.py:419-435, ``visualize_poisson_integration``): the displacement field integrated into the density-gradient image.

The reference solves the Poisson equation on the interior with two-dimensional orthonormal DSTs in float64 on the host.  Here the
same transforms run as four fp64 matrix-core GEMMs per batch (csrc/poisson.hip): with h = H - 2, w = W - 2,

    P = S_h^T ((S_h F S_w^T) / D) S_w,

F the interior divergence of the flow minus the boundary's 5-point stencil, S_N the orthonormal DST-II matrix and D the
eigenvalues of the 5-point Laplacian.  The result is the boundary image with its interior replaced by P.  The differences that form
F are taken in the flow's dtype and summed in float64, as in the reference; every product is float64.  An item's result has the same
bits alone or in a batch and from run to run.

``poisson_reconstruct`` and ``standardize_image_center`` have the reference's names, parameters and dtype rules (the result has
the boundary's dtype).  ``poisson_reconstruct_batch`` integrates a batch without a host synchronisation; ``poisson_image`` returns
the uint8 picture that ``visualize_poisson_integration`` hands to PIL.

Deliberate differences from the reference:
  - an all-zero field gives a uint8 image of 128 everywhere (the reference divides 0 by 0 and casts NaN);
  - P agrees with the reference to about 1e-14 of max|P|, not bit for bit (matrix products instead of FFTs), so a uint8 pixel
    whose unrounded value lies within that distance of an integer can differ by one;
  - flows and boundaries must be float32 or float64 and H, W >= 3; anything else raises ``ValueError``;
  - there is no CPU computation: numpy arrays and CPU tensors are uploaded, and without a GPU the call raises
    ``HipUnavailableError``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import check, stream_ptr
from ._staging import default_device

_DTYPES = {torch.float32: _hip.POISSON_F32, torch.float64: _hip.POISSON_F64}


def _as_device_tensor(x, name: str, device: Optional[torch.device]) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        if any(s < 0 for s in x.strides):
            x = np.ascontiguousarray(x)
        x = torch.from_numpy(x)
    elif not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(x).__name__}")
    if x.dtype not in _DTYPES:
        raise ValueError(f"{name} must be float32 or float64, got {x.dtype}")
    if not x.is_cuda:
        x = x.to(device or default_device())
    return x


def _unit_columns(x: torch.Tensor) -> torch.Tensor:
    """A view the kernel reads in place (unit column stride, non-negative strides), else a contiguous copy."""
    if (x.stride(-1) != 1 and x.shape[-1] != 1) or any(s < 0 for s in x.stride()):
        x = x.contiguous()
    return x


def _launch(flow: torch.Tensor, sc: int, boundary: Optional[torch.Tensor], out_dtype: torch.dtype, want_image: bool
            ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """flow: device [B, *, H, W] with gradx at component 0 and grady ``sc`` elements further; boundary: None or [B', H, W] (B' in
    {1, B}) of ``out_dtype``.  -> (P [B, H, W] of out_dtype, uint8 [B, H, W] or None)."""
    lib = _hip.require_gpu()
    B, H, W = int(flow.shape[0]), int(flow.shape[-2]), int(flow.shape[-1])
    dev = flow.device
    out = torch.empty((B, H, W), dtype=out_dtype, device=dev)
    img = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_image else None
    scratch = torch.empty(int(lib.ebos_poisson_scratch_bytes(B, H, W)), dtype=torch.uint8, device=dev)
    if boundary is not None:
        b_ptr, b_sb, b_sr = boundary.data_ptr(), (boundary.stride(0) if boundary.shape[0] > 1 else 0), boundary.stride(1)
    else:
        b_ptr, b_sb, b_sr = None, 0, 0
    with _hip.on_device(dev):
        check(lib.ebos_poisson_reconstruct(_DTYPES[flow.dtype], _DTYPES[out_dtype], B, H, W, flow.data_ptr(), flow.stride(0), sc,
                                           flow.stride(-2), b_ptr, b_sb, b_sr, out.data_ptr(), out.stride(0), out.stride(1),
                                           None if img is None else img.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                           stream_ptr(dev)), "ebos_poisson_reconstruct")
    return out, img


def _dtype_of(x) -> torch.dtype:
    return x.dtype if isinstance(x, torch.Tensor) else torch.from_numpy(np.zeros(0, dtype=x.dtype)).dtype


def _prepare_batch(flow, boundary, dtype):
    """-> (flow [B, 2, H, W] device view, boundary [B', H, W] device view or None, output dtype).  Everything is validated before
    anything is uploaded."""
    if not isinstance(flow, (np.ndarray, torch.Tensor)):
        raise ValueError(f"flow must be a numpy array or a torch tensor, got {type(flow).__name__}")
    if flow.ndim == 3:
        flow = flow[None]
    if flow.ndim != 4 or flow.shape[1] != 2 or flow.shape[0] == 0:
        raise ValueError(f"flow must be [B, 2, H, W] or [2, H, W] with B > 0, got shape {tuple(flow.shape)}")
    B, _, H, W = (int(v) for v in flow.shape)
    if H < 3 or W < 3:
        raise ValueError(f"Poisson integration needs H, W >= 3, got {H} x {W}")
    if _dtype_of(flow) not in _DTYPES:
        raise ValueError(f"flow must be float32 or float64, got {flow.dtype}")
    if boundary is not None:
        if not isinstance(boundary, (np.ndarray, torch.Tensor)):
            raise ValueError(f"boundary must be a numpy array or a torch tensor, got {type(boundary).__name__}")
        if boundary.ndim == 2:
            boundary = boundary[None]
        if boundary.ndim != 3 or tuple(boundary.shape[1:]) != (H, W) or boundary.shape[0] not in (1, B):
            raise ValueError(f"boundary must be [H, W], [1, H, W] or [B, H, W] = {(B, H, W)}, got {tuple(boundary.shape)}")
        out_dtype = _dtype_of(boundary)
        if dtype is not None and dtype != out_dtype:
            raise ValueError(f"dtype {dtype} differs from the boundary's {out_dtype} (the result has the boundary's dtype)")
    else:
        out_dtype = _dtype_of(flow) if dtype is None else dtype
    if out_dtype not in _DTYPES:
        raise ValueError(f"the output dtype must be float32 or float64, got {out_dtype}")
    f = _unit_columns(_as_device_tensor(flow, "flow", None))
    bnd = None
    if boundary is not None:
        bnd = _unit_columns(_as_device_tensor(boundary, "boundary", f.device))
        if bnd.device != f.device:
            bnd = bnd.to(f.device)
    return f, bnd, out_dtype


def poisson_reconstruct_batch(flow, boundary=None, *, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Integrate every flow of a batch: ``poisson_reconstruct(flow[b, 1], flow[b, 0], boundary[b])`` for all b, in one call and
    without a host synchronisation.

    Args:
        flow ... [B, 2, H, W] or [2, H, W] float32 / float64 (numpy or torch; uploaded when not on the GPU).  Views with a unit
            column stride are read in place; other views are copied first.
        boundary ... None (zeros), or [H, W], [1, H, W] or [B, H, W] float32 / float64: the boundary condition; its dtype is the
            result's (the reference's rule).
        dtype ... the result's dtype when ``boundary`` is None (default: the flow's, as ``np.zeros_like(flow[0])`` gives).

    Returns:
        P: [B, H, W] device tensor.
    """
    f, bnd, out_dtype = _prepare_batch(flow, boundary, dtype)
    return _launch(f, f.stride(1), bnd, out_dtype, False)[0]


def poisson_image(flow, boundary=None, *, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The uint8 picture of ``visualize_poisson_integration`` for every flow of a batch:
    ``standardize_image_center(poisson_reconstruct(flow[1], flow[0], zeros_like(flow[0]))).astype(np.uint8)``, computed in the
    result's dtype.  flow: [B, 2, H, W] or [2, H, W]; boundary / dtype as for ``poisson_reconstruct_batch``.
    Returns a uint8 device tensor [B, H, W]."""
    f, bnd, out_dtype = _prepare_batch(flow, boundary, dtype)
    return _launch(f, f.stride(1), bnd, out_dtype, True)[1]


def _same_storage_offset(gradx: torch.Tensor, grady: torch.Tensor) -> Optional[int]:
    """Element offset of grady from gradx when both are views of one buffer with equal strides and grady lies after gradx."""
    if gradx.dtype != grady.dtype or gradx.device != grady.device or gradx.stride() != grady.stride():
        return None
    if gradx.untyped_storage().data_ptr() != grady.untyped_storage().data_ptr():
        return None
    d = grady.data_ptr() - gradx.data_ptr()
    es = gradx.element_size()
    return d // es if d >= 0 and d % es == 0 else None


def poisson_reconstruct(grady, gradx, boundarysrc):
    """src/utils/stat_utils.py:142-199.  grady, gradx, boundarysrc: [H, W]; the result is ``boundarysrc`` with its interior
    replaced by the Poisson integration of (gradx, grady), in boundarysrc's dtype.  numpy in -> numpy out (uploaded, integrated on
    the GPU, read back); tensors in -> a device tensor out."""
    arrays = (grady, gradx, boundarysrc)
    names = ("grady", "gradx", "boundarysrc")
    for name, a in zip(names, arrays):
        if not isinstance(a, (np.ndarray, torch.Tensor)):
            raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(a).__name__}")
        if a.ndim != 2:
            raise ValueError(f"{name} must be [H, W], got shape {tuple(a.shape)}")
    if not (tuple(grady.shape) == tuple(gradx.shape) == tuple(boundarysrc.shape)):
        raise ValueError(f"grady {tuple(grady.shape)}, gradx {tuple(gradx.shape)} and boundarysrc {tuple(boundarysrc.shape)} "
                         "must have one shape")
    H, W = (int(v) for v in grady.shape)
    if H < 3 or W < 3:
        raise ValueError(f"Poisson integration needs H, W >= 3, got {H} x {W}")
    for name, a in zip(names, arrays):
        if _dtype_of(a) not in _DTYPES:
            raise ValueError(f"{name} must be float32 or float64, got {a.dtype}")
    numpy_out = isinstance(boundarysrc, np.ndarray)
    dev = next((a.device for a in arrays if isinstance(a, torch.Tensor) and a.is_cuda), None)
    gy, gx = _as_device_tensor(grady, "grady", dev), _as_device_tensor(gradx, "gradx", dev)
    dev = gx.device
    if gy.device != dev:
        gy = gy.to(dev)
    bnd = _unit_columns(_as_device_tensor(boundarysrc, "boundarysrc", dev))
    if bnd.device != dev:
        bnd = bnd.to(dev)
    gy, gx = _unit_columns(gy), _unit_columns(gx)
    sc = _same_storage_offset(gx, gy)
    if sc is not None:   # e.g. the component views flow[1], flow[0] of one device [2, H, W] tensor: read in place
        flow = gx.as_strided((1, 2, H, W), (0, sc, gx.stride(0), gx.stride(1)))
    else:
        dtype = torch.promote_types(gx.dtype, gy.dtype)
        flow = torch.stack([gx.to(dtype), gy.to(dtype)])[None]
        sc = flow.stride(1)
    out = _launch(flow, sc, bnd[None], bnd.dtype, False)[0][0]
    return out.cpu().numpy() if numpy_out else out


def standardize_image_center(array, old_center: float = 0, new_center: float = 128, new_max: float = 255):
    """src/utils/frame_utils.py:39-53: ``(array - old_center) / max|array| * (new_max - new_center) + new_center``, dtype kept.
    numpy arrays and tensors (on any device)."""
    if isinstance(array, torch.Tensor):
        max_abs = array.abs().max()
    else:
        max_abs = np.abs(array).max()
    return (array - old_center) / max_abs * (new_max - new_center) + new_center
