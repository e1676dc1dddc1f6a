"""The reference's time-aware flow on the GPU (reference: src/utils/flow_utils.py:49-702; kernels: csrc/flow_voxel.hip): one dense
flow at t0 becomes a flow per time bin.

    construct_dense_flow_voxel_numpy / _torch      [(B,) 2, H, W] -> [(B,) T, 2, H, W], scheme upwind | burgers | same | bilinear
    upwind_flow_to_voxel_numpy / _torch            one first-order upwind step
    inviscid_burger_flow_to_voxel_numpy / _torch   one step with the conservative form of u u_x and v v_y
    propagate_flow_to_voxel_numpy / _torch         "same" (a copy) and "bilinear" (every pixel votes its flow forward)
    truncate_voxel_flow_numpy                      [T, 2, H, W] -> [2, H, W], the masked mean over the bins
    convert_flow_per_bin_to_flow_per_sec           flow / time_scale (plain torch)
    flow_voxel_batch                               the device-only form the constructors call: B flows in the launches of one

flow[0] moves along the rows (the reference's x), flow[1] along the columns.  The advection kernels evaluate the reference's
expressions in its order with every operation rounded on its own, so a step and a chain of steps are the reference's bit for bit,
float32 and float64; the bilinear votes are the reference's addends, summed by float atomics in a free order.  numpy in, numpy out;
a tensor comes back on its device (a CUDA tensor without any host synchronisation).

``flow_voxel_batch`` and the ``_torch`` functions are differentiable with respect to the flow, as the reference's torch expressions are
(kernels: csrc/flow_voxel_grad.hip): a flow that requires grad, with grad mode on, gives a result with a ``grad_fn`` whose backward is
the hand-written adjoint -- torch's rules, half the gradient on each side of a tie of ``maximum`` / ``minimum``, none through ``sign``
and ``floor``, the clamp's bounds included -- gathered without atomics, so two runs give the same bits.  With a clamp the unclamped
voxel is kept for the backward (the steps run on unclamped values).  ``out=`` cannot be combined with such a flow (``ValueError``);
a second derivative raises.  Any other input takes the plain path and its result is what it was.

Reference kinks, each either kept or replaced:

kept
  * ``dt == 0``: the step functions return the input object itself.
  * The step functions and ``propagate_flow_to_voxel_*`` end in ``squeeze()``: every size-1 axis goes, so B = 1, H = 1 or W = 1
    change the rank of what they return.
  * The upwind step divides ``u_dy`` by ``dx`` and ``v_dx``, ``v_dy`` by ``dy``; the Burgers step ``u_dy`` by ``dx`` and ``v_dx`` by ``dy``.
  * The torch Burgers constructor runs its backward loop one step too far (``range(t0_index, -1, -1)``) and stores that step in
    bin ``-1``.  Wherever a forward step follows, it overwrites the bin; where none does -- ``t0_index == time_bin - 1``, which is
    ``time_bin == 1`` and ``time_bin == 2`` with ``t0_location="middle"`` -- the last bin ends as ``t0_index + 1`` backward steps of
    the input (for ``time_bin == 1``: one backward step with dt = 1 instead of the input).  ``construct_dense_flow_voxel_torch``
    reproduces this; the numpy constructor, whose loop stops at 1, does not, and neither does ``flow_voxel_batch`` unless asked.
  * NaN goes through ``np.maximum`` / ``np.minimum`` / ``np.clip`` as in numpy and torch: it propagates.
  * The bilinear vote pairs its four weights with its four cells in the reference's order, in which the second and third weight
    are swapped against the cells: (x1 + 1, y1) gets (1 - fx) fy and (x1, y1 + 1) gets fx (1 - fy).  ``floor(. + 1e-8)`` is kept,
    and a vote outside the image adds ``value * 0`` to cell 0.
  * ``truncate_voxel_flow_numpy`` keeps the ``+ 1e-6`` of its denominator and raises ``NotImplementedError`` for anything but a 4-D
    voxel and ``scheme="mean"``.

replaced (documented exceptions)
  * The constructors keep the rank: a 3-D flow gives 4-D, a 4-D batch 5-D, whatever H and W are.  The reference assigns the
    squeezed step into a bin and fails to broadcast for H = 1 or W = 1.
  * The constructors' ``same`` and ``bilinear`` work, per flow of the batch.  The reference's hand the 4-D batch to
    ``propagate_flow_to_voxel_*``, which unpacks three dimensions and raises for every input.
  * ``max`` needs torch_scatter, ``nearest`` / ``linear`` / ``cubic`` are scipy's ``griddata`` on the host: ``NotImplementedError``
    naming that.  Any other scheme raises ``NotImplementedError`` as in the reference.
  * The ``_numpy`` functions compute and return float64 whatever the input's dtype (the reference's numpy constructor allocates
    ``np.zeros``; its step functions multiply by a ``np.float64`` sign, which numpy >= 2 promotes to float64).  The ``_torch``
    functions keep float32 and float64 and compute everything else in float64.
  * A non-finite bilinear vote (NaN or Inf flow) makes the reference fail on an integer conversion; here it adds NaN to cell 0.
    Cell indices are integers here; the reference's float32 index arithmetic is exact below 2^24 pixels only.
  * ``truncate_voxel_flow_numpy`` asks for two flow components in axis 1 (``ValueError`` otherwise).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _hip, _staging
from ._hip import check, ptr, stream_ptr

_ADVECT = {"upwind": _hip.FLOW_UPWIND, "burgers": _hip.FLOW_BURGERS, "same": _hip.FLOW_SAME}
_UNPORTED = {"max": "it needs torch_scatter's scatter_max in the reference",
             "nearest": "it is scipy.interpolate.griddata on the host in the reference",
             "linear": "it is scipy.interpolate.griddata on the host in the reference",
             "cubic": "it is scipy.interpolate.griddata on the host in the reference"}
_FORCE_ROUTE: Optional[int] = None   # tests: _hip.FLOW_ROUTE_FUSED / FLOW_ROUTE_STEPS instead of the kernel's own choice


def halo_cap() -> int:
    """Steps per direction up to which a voxel is one launch (``ebos_flow_voxel_halo_cap``); beyond it every step is a launch."""
    return int(_hip.load_library().ebos_flow_voxel_halo_cap())


def _check_scheme(scheme: str) -> None:
    if scheme in _UNPORTED:
        raise NotImplementedError(f"scheme {scheme!r} is not ported: {_UNPORTED[scheme]}")
    if scheme not in _ADVECT and scheme != "bilinear":
        raise NotImplementedError(f"unknown scheme {scheme!r}: 'upwind', 'burgers', 'same' and 'bilinear' exist")


def _t0_index(t0_location: str, time_bin: int) -> int:
    if t0_location not in ("first", "middle"):
        raise NotImplementedError(f"t0_location must be 'first' or 'middle', got {t0_location!r}")
    return 0 if t0_location == "first" else time_bin // 2


def _check_arguments(time_bin, scheme: str, t0_location: str) -> int:
    """The reference's order: t0_location, then the scheme; -> time_bin as an int."""
    _t0_index(t0_location, 1)
    _check_scheme(scheme)
    if isinstance(time_bin, bool) or not isinstance(time_bin, (int, np.integer)) or time_bin < 1:
        raise ValueError(f"time_bin must be a positive integer, got {time_bin!r}")
    return int(time_bin)


def flow_voxel_batch(flows: torch.Tensor, time_bin: int, scheme: str = "upwind", t0_location: str = "middle", clamp=None,
                     out: Optional[torch.Tensor] = None, *, torch_burgers_wrap: bool = False) -> torch.Tensor:
    """The flow voxels of B flows in the launches of one, on the device, nothing read back.

    Args:
        flows ... [B, 2, H, W] float32 or float64 on the GPU, for instance what ``estimate_batch`` returns.
        time_bin ... T, the bins of a voxel.
        scheme ... 'upwind', 'burgers', 'same' or 'bilinear'.
        t0_location ... 'first': bin 0 is t = 0 and bin T - 1 is t = (T - 1) / T; 'middle': bin T // 2 is t = 0.
        clamp ... if given, the voxel is clamped to [-clamp, clamp] (the steps run on unclamped values).
        out ... [B, T, 2, H, W] of the flows' dtype and device, contiguous and sharing no memory with ``flows``, to fill instead of a
            new tensor.
        torch_burgers_wrap ... reproduce the extra backward step of the reference's torch Burgers constructor (module docstring).

    Returns:
        [B, T, 2, H, W] in the flows' dtype."""
    T = _check_arguments(time_bin, scheme, t0_location)
    t0 = _t0_index(t0_location, T)
    if not isinstance(flows, torch.Tensor) or flows.dim() != 4 or flows.shape[1] != 2:
        raise ValueError(f"flows must be a [B, 2, H, W] tensor, got {tuple(getattr(flows, 'shape', ()))}")
    B, _, H, W = (int(v) for v in flows.shape)
    if min(B, H, W) < 1:
        raise ValueError(f"flows must not be empty, got {tuple(flows.shape)}")
    if not flows.is_cuda:
        raise ValueError("flows must be on the GPU")
    if clamp is not None and math.isnan(float(clamp)):
        raise ValueError("clamp must be a number")
    _hip.suffix(flows.dtype)
    if B * T > 65535 and scheme == "bilinear":
        raise ValueError(f"{B} flows x {T} bins: at most 65535 bins per call")
    if B > 32767 and scheme != "bilinear":
        raise ValueError(f"{B} flows: at most 32767 per call")
    wrap = bool(torch_burgers_wrap) and scheme == "burgers"
    if flows.requires_grad and torch.is_grad_enabled():
        if out is not None:
            raise ValueError("out= cannot be filled for flows that require grad: the voxel has to be a new tensor of the graph")
        if scheme == "bilinear":
            return _BilinearVoxel.apply(flows, T, t0, T, 0.0, clamp)
        return _AdvectVoxel.apply(flows, T, scheme, t0, clamp, wrap)
    dev = flows.device
    src = flows.detach().contiguous()
    with _hip.on_device(dev):
        if out is None:
            out = torch.empty((B, T, 2, H, W), dtype=flows.dtype, device=dev)
        elif (tuple(out.shape) != (B, T, 2, H, W) or out.dtype != flows.dtype or out.device != dev or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {flows.dtype} tensor of shape {(B, T, 2, H, W)} on {dev}")
        lo, hi = src.data_ptr(), src.data_ptr() + src.numel() * src.element_size()
        if out.data_ptr() < hi and lo < out.data_ptr() + out.numel() * out.element_size():
            raise ValueError("out must not overlap the flows' memory: the bins are written while the flows are still read")
        if scheme == "bilinear":
            _launch_bilinear(src, out, t0, T, 0.0, clamp)
        else:
            _launch_advect(src, out, scheme, t0, clamp, wrap)
    return out


def _launch_advect(src: torch.Tensor, out: torch.Tensor, scheme: str, t0: int, clamp, wrap: bool) -> None:
    """out [B, T, 2, H, W] = the voxel of src [B, 2, H, W], on the current device."""
    B, T, _, H, W = (int(v) for v in out.shape)
    route = _hip.FLOW_ROUTE_AUTO if _FORCE_ROUTE is None else _FORCE_ROUTE
    check(getattr(_hip.require_gpu(), "ebos_flow_voxel_advect_" + _hip.suffix(src.dtype))(
        _ADVECT[scheme], B, T, H, W, ptr(src), ptr(out), t0, int(clamp is not None), float(clamp if clamp is not None else 0.0), int(wrap), route,
        stream_ptr(src.device)), "ebos_flow_voxel_advect")


def _launch_bilinear(src: torch.Tensor, out: torch.Tensor, t_offset: int, denominator: int, dt: float, clamp) -> None:
    """out [B, T, 2, H, W]: bin t is src [B, 2, H, W] carried along itself for (t - t_offset) / denominator, or for dt with denominator 0."""
    B, T, _, H, W = (int(v) for v in out.shape)
    check(getattr(_hip.require_gpu(), "ebos_flow_voxel_propagate_bilinear_" + _hip.suffix(src.dtype))(
        B, T, H, W, ptr(src), ptr(out), t_offset, denominator, float(dt), int(clamp is not None), float(clamp if clamp is not None else 0.0),
        stream_ptr(src.device)), "ebos_flow_voxel_propagate_bilinear")


def _clamped_copy(raw: torch.Tensor, clamp) -> torch.Tensor:
    out = torch.empty_like(raw)
    check(getattr(_hip.require_gpu(), "ebos_flow_voxel_clamp_" + _hip.suffix(raw.dtype))(raw.numel(), ptr(raw), ptr(out), float(clamp),
                                                                                         stream_ptr(raw.device)), "ebos_flow_voxel_clamp")
    return out


# The backward with respect to the flow (csrc/flow_voxel_grad.hip).  The steps of a chain run on unclamped values and the clamp comes
# last, so with a clamp the forward keeps the unclamped voxel -- the chain's intermediates, and what the clamp's mask is taken from --
# and returns a clamped copy.  Double backward is not supported: once_differentiable raises on it.
class _AdvectVoxel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, T, scheme, t0, clamp, wrap):
        src = flows.detach().contiguous()
        B, _, H, W = (int(v) for v in src.shape)
        keep = scheme != "same"
        with _hip.on_device(src.device):
            out = torch.empty((B, T, 2, H, W), dtype=src.dtype, device=src.device)
            _launch_advect(src, out, scheme, t0, None if keep else clamp, wrap)
            raw = out if keep else None
            if keep and clamp is not None:
                out = _clamped_copy(raw, clamp)
        ctx.save_for_backward(src, raw)
        ctx.meta = (T, scheme, t0, clamp, wrap)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        src, raw = ctx.saved_tensors
        T, scheme, t0, clamp, wrap = ctx.meta
        lib = _hip.require_gpu()
        B, _, H, W = (int(v) for v in src.shape)
        g = g.contiguous()
        route = _hip.FLOW_ROUTE_AUTO if _FORCE_ROUTE is None else _FORCE_ROUTE
        with _hip.on_device(src.device):
            d = torch.empty_like(src)
            n = int(lib.ebos_flow_voxel_advect_adjoint_workspace(_ADVECT[scheme], B, T, H, W, t0, int(wrap), route))
            if n < 0:
                raise RuntimeError("ebos_flow_voxel_advect_adjoint_workspace: " + lib.ebos_last_error().decode("utf-8", "replace"))
            ws = torch.empty(n, dtype=src.dtype, device=src.device) if n else None
            check(getattr(lib, "ebos_flow_voxel_advect_adjoint_" + _hip.suffix(src.dtype))(
                _ADVECT[scheme], B, T, H, W, ptr(src), ptr(raw), ptr(g), ptr(d), t0, int(clamp is not None),
                float(clamp if clamp is not None else 0.0), int(wrap), route, ptr(ws), stream_ptr(src.device)), "ebos_flow_voxel_advect_adjoint")
        return d, None, None, None, None, None


class _BilinearVoxel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, T, t_offset, denominator, dt, clamp):
        src = flows.detach().contiguous()
        B, _, H, W = (int(v) for v in src.shape)
        with _hip.on_device(src.device):
            out = torch.empty((B, T, 2, H, W), dtype=src.dtype, device=src.device)
            _launch_bilinear(src, out, t_offset, denominator, dt, None)
            raw = out if clamp is not None else None
            if clamp is not None:
                out = _clamped_copy(raw, clamp)
        ctx.save_for_backward(src, raw)
        ctx.meta = (T, t_offset, denominator, dt, clamp)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        src, raw = ctx.saved_tensors
        T, t_offset, denominator, dt, clamp = ctx.meta
        B, _, H, W = (int(v) for v in src.shape)
        g = g.contiguous()
        with _hip.on_device(src.device):
            d = torch.empty_like(src)
            check(getattr(_hip.require_gpu(), "ebos_flow_voxel_propagate_bilinear_adjoint_" + _hip.suffix(src.dtype))(
                B, T, H, W, ptr(src), ptr(raw), ptr(g), ptr(d), t_offset, denominator, float(dt), int(clamp is not None),
                float(clamp if clamp is not None else 0.0), stream_ptr(src.device)), "ebos_flow_voxel_propagate_bilinear_adjoint")
        return d, None, None, None, None, None


class _Step(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, name, dt, dx, dy):
        src = flows.detach().contiguous()
        ctx.save_for_backward(src)
        ctx.meta = (name, dt, dx, dy)
        return _launch_step(name, src, dt, dx, dy)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (src,) = ctx.saved_tensors
        name, dt, dx, dy = ctx.meta
        B, _, H, W = (int(v) for v in src.shape)
        g = g.contiguous()
        with _hip.on_device(src.device):
            d = torch.empty_like(src)
            check(getattr(_hip.require_gpu(), f"ebos_flow_{name}_step_adjoint_" + _hip.suffix(src.dtype))(
                B, H, W, ptr(src), ptr(g), ptr(d), dt, dx, dy, stream_ptr(src.device)), f"ebos_flow_{name}_step_adjoint")
        return d, None, None, None, None


def _launch_step(name: str, src: torch.Tensor, dt: float, dx: float, dy: float) -> torch.Tensor:
    B, _, H, W = (int(v) for v in src.shape)
    with _hip.on_device(src.device):
        out = torch.empty_like(src)
        check(getattr(_hip.require_gpu(), f"ebos_flow_{name}_step_" + _hip.suffix(src.dtype))(B, H, W, ptr(src), ptr(out), dt, dx, dy,
                                                                                            stream_ptr(src.device)), f"ebos_flow_{name}_step")
    return out


def _construct(dense_flow, time_bin, scheme, t0_location, clamp, kind, wrap):
    _check_arguments(time_bin, scheme, t0_location)
    if len(dense_flow.shape) not in (3, 4):
        raise ValueError(f"dense_flow must be [2, H, W] or [B, 2, H, W], got {tuple(dense_flow.shape)}")
    single = len(dense_flow.shape) == 3
    dev = dense_flow.device if kind == _staging.GPU else None
    flows = _staging.to_gpu(dense_flow, dev, torch.float64 if kind == _staging.NUMPY else None)
    voxel = flow_voxel_batch(flows[None] if single else flows, time_bin, scheme, t0_location, clamp, torch_burgers_wrap=wrap)
    return _staging.back(voxel[0] if single else voxel, kind)


def construct_dense_flow_voxel_numpy(dense_flow: np.ndarray, time_bin: int, scheme: str = "upwind", t0_location: str = "middle",
                                     clamp: Optional[int] = None) -> np.ndarray:
    """The flow voxel of one flow or a batch of flows, computed on the GPU (reference: src/utils/flow_utils.py:97-159).

    ``dense_flow`` is ``[2, H, W]`` or ``[B, 2, H, W]`` and holds the flow at t0; the result has ``time_bin`` bins in a new axis in front
    of the components, ``[(B,) time_bin, 2, H, W]``, always float64.  ``scheme`` is one of 'upwind', 'burgers', 'same', 'bilinear'.
    ``t0_location`` says which bin is the input: 'first' puts it in bin 0, and bin s is then s steps of 1 / time_bin later; 'middle'
    puts it in bin ``time_bin // 2`` with the earlier times below it and the later ones above.  With ``clamp`` the finished voxel is
    limited to ``[-clamp, clamp]``."""
    if not isinstance(dense_flow, np.ndarray):
        raise TypeError(f"construct_dense_flow_voxel_numpy takes a numpy array, got {type(dense_flow).__name__}")
    return _construct(dense_flow, time_bin, scheme, t0_location, clamp, _staging.NUMPY, False)


def construct_dense_flow_voxel_torch(dense_flow: torch.Tensor, time_bin: int, scheme: str = "upwind", t0_location: str = "middle",
                                     clamp: Optional[int] = None) -> torch.Tensor:
    """``construct_dense_flow_voxel_numpy`` for tensors (src/utils/flow_utils.py:162-224): the voxel comes back on the flow's device
    in its dtype (float32 and float64 are kept), a CUDA tensor without any host synchronisation.  With scheme 'burgers' the last bin
    carries the reference's extra backward step where ``t0_index == time_bin - 1`` (module docstring)."""
    if not isinstance(dense_flow, torch.Tensor):
        raise TypeError(f"construct_dense_flow_voxel_torch takes a tensor, got {type(dense_flow).__name__}")
    return _construct(dense_flow, time_bin, scheme, t0_location, clamp, _staging.kind_of(dense_flow), True)


def _step(name: str, flow, dt: float, dx, dy, kind: str):
    if dt == 0:
        return flow
    if len(flow.shape) not in (3, 4) or flow.shape[-3] != 2:
        raise ValueError(f"flow must be [2, H, W] or [B, 2, H, W], got {tuple(flow.shape)}")
    if any(math.isnan(float(v)) for v in (dt, dx, dy)):
        raise ValueError(f"dt, dx and dy must be numbers, got {dt!r}, {dx!r}, {dy!r}")
    if min(int(v) for v in flow.shape) < 1:
        raise ValueError(f"flow must not be empty, got {tuple(flow.shape)}")
    _hip.require_gpu()
    dev = flow.device if kind == _staging.GPU else None
    src = _staging.to_gpu(flow, dev, torch.float64 if kind == _staging.NUMPY else None)
    if src.dim() == 3:
        src = src[None]
    if int(src.shape[0]) > 32767:
        raise ValueError(f"{int(src.shape[0])} flows: at most 32767 per call")
    if src.requires_grad and torch.is_grad_enabled():
        out = _Step.apply(src, name, float(dt), float(dx), float(dy))
    else:
        out = _launch_step(name, src.detach().contiguous(), float(dt), float(dx), float(dy))
    return _staging.back(out.squeeze(), kind)


def _numpy_only(a, who: str):
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{who} takes a numpy array, got {type(a).__name__}")


def _torch_only(a, who: str):
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{who} takes a tensor, got {type(a).__name__}")


def upwind_flow_to_voxel_numpy(flow: np.ndarray, dt: float, dx: int = 1, dy: int = 1) -> np.ndarray:
    """One first-order upwind step of the flow's self-advection (reference: src/utils/flow_utils.py:447-499).

    ``flow`` is ``[2, H, W]`` or ``[B, 2, H, W]``.  A positive ``dt`` advances the flow by that time; a negative one steps the negated flow
    by ``|dt|`` and negates the result; 0 hands back ``flow`` itself.  ``dx`` divides both differences of flow[0] and ``dy`` both of
    flow[1].  The result is float64 and has lost its size-1 axes."""
    _numpy_only(flow, "upwind_flow_to_voxel_numpy")
    return _step("upwind", flow, dt, dx, dy, _staging.NUMPY)


def upwind_flow_to_voxel_torch(flow: torch.Tensor, dt: float, dx: int = 1, dy: int = 1) -> torch.Tensor:
    """``upwind_flow_to_voxel_numpy`` for tensors (src/utils/flow_utils.py:502-556), in the flow's dtype on its device."""
    _torch_only(flow, "upwind_flow_to_voxel_torch")
    return _step("upwind", flow, dt, dx, dy, _staging.kind_of(flow))


def inviscid_burger_flow_to_voxel_numpy(flow: np.ndarray, dt: float, dx: int = 1, dy: int = 1) -> np.ndarray:
    """One step in which u u_x and v v_y take the conservative form of the inviscid Burgers equation and the cross terms stay upwind
    differences (reference: src/utils/flow_utils.py:559-627).

    ``flow``, the sign of ``dt`` and ``dt == 0`` as in ``upwind_flow_to_voxel_numpy``.  ``dx`` divides the column difference of flow[0],
    ``dy`` the row difference of flow[1].  The result is float64 and has lost its size-1 axes."""
    _numpy_only(flow, "inviscid_burger_flow_to_voxel_numpy")
    return _step("burgers", flow, dt, dx, dy, _staging.NUMPY)


def inviscid_burger_flow_to_voxel_torch(flow: torch.Tensor, dt: float, dx: int = 1, dy: int = 1) -> torch.Tensor:
    """``inviscid_burger_flow_to_voxel_numpy`` for tensors (src/utils/flow_utils.py:630-702), in the flow's dtype on its device."""
    _torch_only(flow, "inviscid_burger_flow_to_voxel_torch")
    return _step("burgers", flow, dt, dx, dy, _staging.kind_of(flow))


def _propagate(flow_0, dt: float, method: str, kind: str):
    if method in _UNPORTED:
        raise NotImplementedError(f"method {method!r} is not ported: {_UNPORTED[method]}")
    if method not in ("same", "bilinear"):
        raise NotImplementedError(f"unknown method {method!r}: 'same' and 'bilinear' exist")
    if len(flow_0.shape) != 3 or flow_0.shape[0] != 2:
        raise ValueError(f"flow_0 must be [2, H, W], got {tuple(flow_0.shape)}")
    if method == "same":
        return np.copy(flow_0).squeeze() if kind == _staging.NUMPY else torch.clone(flow_0).squeeze()
    if not math.isfinite(float(dt)):
        raise ValueError(f"dt must be finite, got {dt!r}")
    _, H, W = (int(v) for v in flow_0.shape)
    if min(H, W) < 1:
        raise ValueError(f"flow_0 must not be empty, got {tuple(flow_0.shape)}")
    _hip.require_gpu()
    dev = flow_0.device if kind == _staging.GPU else None
    src = _staging.to_gpu(flow_0, dev, torch.float64 if kind == _staging.NUMPY else None)
    if src.requires_grad and torch.is_grad_enabled():
        out = _BilinearVoxel.apply(src[None], 1, 0, 0, float(dt), None)[0, 0]
    else:
        src = src.detach().contiguous()
        with _hip.on_device(src.device):
            out = torch.empty_like(src)
            _launch_bilinear(src[None], out[None, None], 0, 0, float(dt), None)
    return _staging.back(out.squeeze(), kind)


def propagate_flow_to_voxel_numpy(flow_0: np.ndarray, dt: float, method: str = "nearest") -> np.ndarray:
    """Carry every pixel's flow along itself for the time ``dt`` (reference: src/utils/flow_utils.py:227-342).

    ``flow_0`` is ``[2, H, W]``; pixel (i, j) lands on (i + flow_0[0] dt, j + flow_0[1] dt).  ``method`` 'bilinear' spreads its flow over
    the four cells around that point, 'same' copies the input.  The default, "nearest", is the reference's default and one of the
    host-side methods that raise ``NotImplementedError`` here (module docstring).  The result has lost its size-1 axes and is float64
    for 'bilinear'."""
    _numpy_only(flow_0, "propagate_flow_to_voxel_numpy")
    return _propagate(flow_0, dt, method, _staging.NUMPY)


def propagate_flow_to_voxel_torch(flow_0: torch.Tensor, dt: float, method: str = "nearest") -> torch.Tensor:
    """``propagate_flow_to_voxel_numpy`` for tensors (src/utils/flow_utils.py:345-444), in the flow's dtype on its device."""
    _torch_only(flow_0, "propagate_flow_to_voxel_torch")
    return _propagate(flow_0, dt, method, _staging.kind_of(flow_0))


def truncate_voxel_flow_numpy(flow_voxel: np.ndarray, scheme: str = "mean") -> np.ndarray:
    """Collapse a flow voxel ``[bins, 2, H, W]`` to one flow ``[2, H, W]``, float64 (reference: src/utils/flow_utils.py:68-93): per pixel
    the mean over the bins whose flow is not zero, ``sum(flow * mask) / (sum(mask) + 1e-6)``, the bins added in index order.  Only
    ``scheme="mean"`` exists."""
    _numpy_only(flow_voxel, "truncate_voxel_flow_numpy")
    if len(flow_voxel.shape) != 4:
        raise NotImplementedError(f"truncate_voxel_flow_numpy takes a 4-D voxel [bins, 2, H, W], got shape {tuple(flow_voxel.shape)}")
    if scheme != "mean":
        raise NotImplementedError(f"truncate_voxel_flow_numpy knows the scheme 'mean' only, got {scheme!r}")
    T, two, H, W = (int(v) for v in flow_voxel.shape)
    if two != 2 or min(T, H, W) < 1:
        raise ValueError(f"flow_voxel must be a non-empty [bin, 2, H, W], got {flow_voxel.shape}")
    lib = _hip.require_gpu()
    src = _staging.to_gpu(flow_voxel).contiguous()
    with _hip.on_device(src.device):
        out = torch.empty((2, H, W), dtype=torch.float64, device=src.device)
        check(getattr(lib, "ebos_flow_voxel_truncate_mean_" + _hip.suffix(src.dtype))(T, H, W, ptr(src), ptr(out), stream_ptr(src.device)),
              "ebos_flow_voxel_truncate_mean")
    return _staging.back(out, _staging.NUMPY)


def convert_flow_per_bin_to_flow_per_sec(flow_per_bin: torch.Tensor, time_scale: torch.Tensor, n_bin: int):
    """Flows ``[B, 2, H, W]`` measured over a whole voxel, divided by the voxel's duration ``time_scale`` ``[B, 1]`` (reference:
    src/utils/flow_utils.py:49-64).  ``n_bin`` is accepted and not used, as there.  Plain torch."""
    return flow_per_bin / time_scale[..., None, None]
