"""The Adam loop of the time-aware patch-flow contrast maximisation (the solver's ``time_aware`` block with ``native: true``) as
one C call, without autograd (kernels: csrc/cmax_voxel.hip, csrc/warp_voxel.hip), for B windows of one geometry in the launches of
one window (``TimeAwarePatchLoopBatch``: ``ebos_cmax_voxel_solve_batch_f32``).  Per window

    loss(theta) = -w var(IWE(events warped by voxel(dense(theta)))) + w_n flow_norm(dense) + w_g image_gradient(dense)

One iteration, on buffers allocated once per loop; every stage takes the window from an outer grid dimension, each window has its
own events, grid and Adam state:

    ebos_upsample_patch_flow_batch_f32           theta [B, 2, gh, gw] -> dense [B, 2, H, W], the flow at t0
    ebos_flow_voxel_advect_f32                   dense -> voxel [B, T, 2, H, W] (upwind | burgers; with a clamp: + the clamped copy)
    memset + ebos_iwe_voxel_tiled_batch_f32      every event displaced by the flow of its own bin -> IWE [B, h, w]
    ebos_image_variance_f32 / _affine_f32        variance, its moments, and its gradient as an affine map of the IWE
    ebos_flow_regularisers_batch_f32             (with a regulariser weight) value partials + gradient image
    ebos_iwe_voxel_owner_bwd_batch_f32           -> d_voxel: the owner of a source pixel's run writes its 2 T cells; no atomics, no clearing
    ebos_flow_voxel_advect_adjoint_f32           -> d_dense (+ the regularisers' gradient)
    ebos_upsample_patch_flow_bwd_adam_batch_f32  -> d_theta, the Adam step of every grid element, loss[b, it]

``owner_bwd=False`` swaps the backward for a memset and the global-atomic ``ebos_iwe_voxel_bwd_f32`` window by window: the two stay
comparable inside one loop; ``owner_bwd=None`` takes whichever was measured faster for the window's size and bins
(``default_owner_bwd``).  The family: the variance contrast alone, optional ``flow_norm`` / ``image_gradient``, no ``iwe.blur_sigma``;
anything else belongs to the autograd loop of ``ContrastMaximization``.

One window is a batch of one, on the same code path: ``TimeAwarePatchLoop`` is the face of a ``TimeAwarePatchLoopBatch`` of B = 1
without the window dimension.

``time_aware.directions`` (K reference times, ``TimeAwareMultiReferencePatchLoopBatch`` and its one-window face): the same loop on
B K images, ``ebos_cmax_voxel_multiref_solve_batch_f32`` --

    loss(theta) = -(w / (K N)) sum_k var(IWE_k(events warped by voxel(dense(theta)), reference time k)) + the regularisers

with ``ebos_iwe_voxel_multiref_tiled_batch_f32`` and ``ebos_iwe_voxel_multiref_owner_bwd_batch_f32`` in the place of the forward and
the backward (an event is loaded and its bin's flow gathered once for all K references; d_voxel is written once), and N the variance
of the window's zero-flow IWE with ``time_aware.normalize`` (1 without it).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _hip
from .._hip import check, ptr, stream_ptr
from ..event_plan import EventPlan, TimeAwarePlanStack, _voxel_halo
from ..flow_voxel import _ADVECT, _t0_index

DEFAULT_TILE = (64, 64)    # the plan tile of a native time-aware solve: a built ebos_tiled_config (the tiled forward kernel)


def default_owner_bwd(time_bin: int, n_events: int) -> bool:
    """Which backward a loop runs when its caller does not say.  Measured per iteration on an MI355X (tools/bench_voxel_loop.py,
    DESIGN 4.22): at 2 M events the owner kernel wins at T = 15 (555 against 585 us) and loses at T = 5 (222.1 against 221.1 us, the
    intervals apart); at 100 k events the atomic kernel wins at both.  The two thresholds are the midpoints between the measured
    points and nothing more."""
    return int(time_bin) >= 10 and int(n_events) >= 1_000_000


class TimeAwarePatchLoopBatch(object):
    """The loop for B windows at once.  Constructor shape of ``fused_loop.FusedPatchLoop`` plus ``time_aware``, the parsed block
    (``parse_time_aware``): ``plans`` is a sequence of binned time-aware plans of one geometry (or a ``TimeAwarePlanStack``), ``theta0``
    [B, 2, gh, gw], ``theta_mask`` [B, gh, gw]; the other arguments hold for every window.  ``owner_bwd=None`` resolves through
    ``default_owner_bwd(T, the largest window)``."""
    graphed = False
    last_run_mode = "native-batch"
    K = None                   # reference times per window (None: one, the plan's own; the image buffers then have no such dimension)
    _SOLVE, _GRADIENT = "ebos_cmax_voxel_solve_batch", "ebos_cmax_voxel_gradient_batch"   # the C entry points, without _f32

    def __init__(self, plans, patch_size: Tuple[int, int], sliding_window: Tuple[int, int], theta0: torch.Tensor,
                 time_aware: dict, w_variance: float = 1.0, w_flow_norm: float = 0.0, w_image_gradient: float = 0.0,
                 omit_boundary: bool = False, pad: int = 0, halo="auto", lr: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 capacity: int = 1024, theta_mask: Optional[torch.Tensor] = None, owner_bwd: Optional[bool] = None):
        self.lib = lib = _hip.require_gpu()
        ta = dict(time_aware)
        self.stack = stack = plans if isinstance(plans, TimeAwarePlanStack) else EventPlan.stack_time_aware(plans)
        self.B = B = len(stack)
        if int(ta["time_bin"]) != stack.time_bin:
            raise ValueError(f"the plans' bins were made for time_bin={stack.time_bin}, time_aware asks for {ta['time_bin']}")
        if ta.get("scheme", "upwind") not in ("upwind", "burgers"):
            raise NotImplementedError(f"time_aware.scheme {ta.get('scheme')!r}: the native loop runs 'upwind' and 'burgers'")
        if float(w_variance) == 0.0:
            raise ValueError("w_variance must be non-zero")
        self.patch, self.slide = tuple(int(v) for v in patch_size), tuple(int(v) for v in sliding_window)
        self.T, self.scheme = int(ta["time_bin"]), _ADVECT[ta.get("scheme", "upwind")]
        self.t0 = _t0_index(ta.get("t0_location", "middle"), self.T)
        self.clamp = None if ta.get("clamp") is None else float(ta["clamp"])
        self.w_var, self.w_norm, self.w_tv = float(w_variance), float(w_flow_norm), float(w_image_gradient)
        self.omit, self.pad = bool(omit_boundary), (int(pad), int(pad))
        built = _voxel_halo(stack.plans[0], halo)       # None: (tile, halo) is no built configuration -> the general forward kernel
        self.halo = 0 if built is None else int(built)
        self.splits = max(1, max(p.resolve_splits(None) for p in stack.plans))
        self.owner_bwd = default_owner_bwd(self.T, max(stack.ns)) if owner_bwd is None else bool(owner_bwd)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        from .. import flow_voxel as _fv

        self.route = _hip.FLOW_ROUTE_AUTO if _fv._FORCE_ROUTE is None else _fv._FORCE_ROUTE
        dev = stack.device
        H, W = stack.image_size
        f32 = dict(dtype=torch.float32, device=dev)
        self.theta = theta0.detach().to(**f32).contiguous().clone()
        if self.theta.dim() != 4 or self.theta.shape[0] != B or self.theta.shape[1] != 2:
            raise ValueError(f"theta0 must be [{B}, 2, gh, gw], got {tuple(theta0.shape)}")
        _, _, self.gh, self.gw = self.theta.shape
        self.theta_mask = None if theta_mask is None else theta_mask.detach().to(**f32).reshape(B, self.gh, self.gw).contiguous()
        self.d_theta = torch.empty_like(self.theta)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t = 0
        self.has_reg = self.w_norm != 0.0 or self.w_tv != 0.0
        self.dense, self.d_dense = torch.empty((B, 2, H, W), **f32), torch.empty((B, 2, H, W), **f32)
        self.d_reg = torch.empty((B, 2, H, W), **f32) if self.has_reg else None
        self.voxel, self.d_voxel = torch.empty((B, self.T, 2, H, W), **f32), torch.empty((B, self.T, 2, H, W), **f32)
        self.voxel_clamped = torch.empty_like(self.voxel) if self.clamp is not None else None
        lead = (B,) if self.K is None else (B, self.K)         # one image per window, or per (window, reference time)
        self.iwe = torch.empty(lead + (H + 2 * self.pad[0], W + 2 * self.pad[1]), **f32)
        self.variance = torch.empty(lead, **f32)
        self.moments = torch.empty(lead + (2,), dtype=torch.float64, device=dev)
        self.upstream = torch.full(lead, -self.w_var / (self.K or 1), **f32)   # loss = -w * (mean) contrast, per window
        self.affine = torch.empty(lead + (2,), **f32)
        self.cost_scratch = torch.empty(int(lib.ebos_cost_scratch_bytes(B * (self.K or 1))), dtype=torch.uint8, device=dev)
        self.n_reg = int(lib.ebos_flow_regularisers_partials()) if self.has_reg else 0
        self.reg_partials = torch.zeros((B, max(self.n_reg, 1)), dtype=torch.float64, device=dev)
        self.scratch_up = torch.empty(B * (int(lib.ebos_upsample_bwd_scratch_bytes(self.gh, W)) // 4), **f32)
        n_ws = int(lib.ebos_flow_voxel_advect_adjoint_workspace(self.scheme, B, self.T, H, W, self.t0, 0, self.route))
        if n_ws < 0:
            raise RuntimeError("ebos_flow_voxel_advect_adjoint_workspace: " + lib.ebos_last_error().decode("utf-8", "replace"))
        self.adjoint_ws = torch.empty(n_ws, **f32) if n_ws else None
        self.losses = torch.zeros((B, max(int(capacity), 1)), **f32)   # [B, capacity]: row b, entry it = window b's loss before update it

    def problem(self) -> "_hip.CmaxVoxelBatchProblem":
        """The loop's buffers as the ``ebos_cmax_voxel_batch_problem`` struct of the C ABI."""
        st = self.stack
        q = _hip.CmaxVoxelBatchProblem()
        q.B = self.B
        q.xs, q.ys, q.dts, q.bins, q.key_offsets = ptr(st.x), ptr(st.y), ptr(st.dt), ptr(st.bins), ptr(st.key_offsets)
        for b, n in enumerate(st.ns):
            q.n[b] = n
        q.H, q.W = st.image_size
        q.tile_h, q.tile_w, q.halo = st.tile[0], st.tile[1], self.halo
        q.pad_h, q.pad_w, q.omit_boundary, q.splits = self.pad[0], self.pad[1], int(self.omit), self.splits
        q.T, q.scheme, q.t0_index, q.wrap_last, q.route = self.T, self.scheme, self.t0, 0, self.route
        q.has_clamp, q.clamp = int(self.clamp is not None), float(self.clamp or 0.0)
        q.owner_bwd = int(self.owner_bwd)
        q.gh, q.gw, (q.patch_h, q.patch_w), (q.slide_h, q.slide_w) = self.gh, self.gw, self.patch, self.slide
        q.w_variance, q.w_flow_norm, q.w_image_gradient = self.w_var, self.w_norm, self.w_tv
        q.lr, q.beta1, q.beta2, q.eps = self.lr, self.betas[0], self.betas[1], self.eps
        q.theta, q.d_theta, q.exp_avg, q.exp_avg_sq = ptr(self.theta), ptr(self.d_theta), ptr(self.exp_avg), ptr(self.exp_avg_sq)
        q.step, q.steps_done = ptr(self.step), self.t
        q.dense, q.d_dense, q.d_reg = ptr(self.dense), ptr(self.d_dense), ptr(self.d_reg)
        q.voxel, q.voxel_clamped, q.d_voxel = ptr(self.voxel), ptr(self.voxel_clamped), ptr(self.d_voxel)
        q.iwe, q.variance, q.moments, q.upstream, q.affine = ptr(self.iwe), ptr(self.variance), ptr(self.moments), ptr(self.upstream), ptr(self.affine)
        q.cost_scratch, q.cost_scratch_bytes = ptr(self.cost_scratch), self.cost_scratch.numel()
        q.reg_partials, q.upsample_scratch = ptr(self.reg_partials), ptr(self.scratch_up)
        q.adjoint_workspace = ptr(self.adjoint_ws)
        q.adjoint_workspace_elems = self.adjoint_ws.numel() if self.adjoint_ws is not None else 0
        q.losses, q.losses_cap, q.theta_mask = ptr(self.losses), self.losses.shape[1], ptr(self.theta_mask)
        return q

    def run(self, n_iter: int) -> torch.Tensor:
        """``n_iter`` more iterations of every window, enqueued by one C call; returns their losses [B, n_iter] (device)."""
        n_iter = int(n_iter)
        if self.t + n_iter > self.losses.shape[1]:
            raise ValueError(f"capacity {self.losses.shape[1]} < {self.t} steps done + {n_iter}")
        t0 = self.t
        with _hip.on_device(self.stack.device):
            check(getattr(self.lib, self._SOLVE + "_f32")(ctypes.byref(self.problem()), n_iter, stream_ptr()), self._SOLVE)
        self.t += n_iter
        return self.losses[:, t0:t0 + n_iter]

    def _contrast(self) -> torch.Tensor:
        """[B]: what the last forward left as every window's contrast."""
        return self.variance

    def value_and_grad(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(losses [B], d loss / d theta [B, 2, gh, gw]) at ``theta`` through the same kernels, without the Adam step."""
        with _hip.on_device(self.stack.device):
            self.theta.copy_(theta.detach().to(self.theta))
            check(getattr(self.lib, self._GRADIENT + "_f32")(ctypes.byref(self.problem()), stream_ptr()), self._GRADIENT)
            loss = -self.w_var * self._contrast()
            if self.n_reg:
                loss = loss + self.reg_partials.sum(dim=1).to(torch.float32)
        return loss, (self.d_theta.clone() if self.theta_mask is None else self.d_theta * self.theta_mask[:, None])


class TimeAwareMultiReferencePatchLoopBatch(TimeAwarePatchLoopBatch):
    """The loop at K reference times: ``time_aware`` carries ``directions`` (1 to 4 reference times, ``multi_reference_fractions``) and
    optionally ``normalize``.  The interface and the buffers are ``TimeAwarePatchLoopBatch``'s with the images per (window, reference):
    ``iwe`` [B, K, h, w], ``variance`` / ``upstream`` [B, K], ``moments`` / ``affine`` [B, K, 2]; ``value`` [B] holds
    ``inv_norm[b] * mean_k variance[b, k]`` and ``inv_norm`` [B] the windows' 1 / N.  Only the owner backward exists for K references."""
    _SOLVE, _GRADIENT = "ebos_cmax_voxel_multiref_solve_batch", "ebos_cmax_voxel_multiref_gradient_batch"

    def __init__(self, plans, patch_size: Tuple[int, int], sliding_window: Tuple[int, int], theta0: torch.Tensor,
                 time_aware: dict, w_variance: float = 1.0, w_flow_norm: float = 0.0, w_image_gradient: float = 0.0,
                 omit_boundary: bool = False, pad: int = 0, halo="auto", lr: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 capacity: int = 1024, theta_mask: Optional[torch.Tensor] = None):
        from ..event_plan import multi_reference_shifts

        ta = dict(time_aware)
        if ta.get("directions") is None:
            raise ValueError("time_aware.directions is missing: the reference times the voxel is scored at")
        stack = plans if isinstance(plans, TimeAwarePlanStack) else EventPlan.stack_time_aware(plans)
        self.shifts = multi_reference_shifts(stack, ta["directions"])   # (ValueError before any buffer is made)
        self.K = K = len(self.shifts)
        # every stage that adds in run order is the owner backward: on the canonical order of a pixel's events two builds of a
        # window's plan give the same d_voxel, bit for bit, and so the same solve
        stack = stack.canonical()
        super().__init__(stack, patch_size, sliding_window, theta0, ta, w_variance, w_flow_norm, w_image_gradient, omit_boundary, pad,
                         halo, lr, betas, eps, capacity, theta_mask, owner_bwd=True)
        lib, B, dev = self.lib, self.B, stack.device
        H, W = stack.image_size
        h, w = H + 2 * self.pad[0], W + 2 * self.pad[1]
        f32 = dict(dtype=torch.float32, device=dev)
        self.inv_norm = torch.ones(B, **f32)
        if ta.get("normalize", False):   # N: the variance of the window's zero-flow IWE (the same image at every reference time)
            iwe0 = torch.zeros((B, h, w), **f32)
            var0 = torch.empty(B, **f32)
            with _hip.on_device(dev):
                self.voxel.zero_()
                check(lib.ebos_iwe_voxel_tiled_batch_f32(ptr(stack.x), ptr(stack.y), ptr(stack.dt), ptr(stack.bins), ptr(stack.key_offsets),
                                                         stack.ns_array(), B, ptr(self.voxel), self.T, H, W, stack.tile[0], stack.tile[1],
                                                         self.halo, self.splits, self.pad[0], self.pad[1], ptr(iwe0), stream_ptr()),
                      "ebos_iwe_voxel_tiled_batch")
                check(lib.ebos_image_variance_f32(ptr(iwe0), B, h, w, int(self.omit), ptr(var0), None, ptr(self.cost_scratch),
                                                  self.cost_scratch.numel(), stream_ptr()), "ebos_image_variance")
            self.inv_norm = torch.where(var0 == 0, torch.ones_like(var0), 1.0 / var0).contiguous()
            self.upstream.mul_(self.inv_norm[:, None])         # loss = -(w / (K N)) sum_k var_k
        self.value = torch.empty(B, **f32)

    def problem(self) -> "_hip.CmaxVoxelMultirefBatchProblem":
        """The loop's buffers as the ``ebos_cmax_voxel_multiref_batch_problem`` struct of the C ABI."""
        base = super().problem()
        q = _hip.CmaxVoxelMultirefBatchProblem()
        for name, _ in _hip.CmaxVoxelMultirefBatchProblem._fields_:
            if hasattr(base, name):
                setattr(q, name, getattr(base, name))
        q.K = self.K
        for k, s in enumerate(self.shifts):
            q.shifts[k] = s
        q.inv_norm, q.value = ptr(self.inv_norm), ptr(self.value)
        return q

    def _contrast(self) -> torch.Tensor:
        return self.value


class _OneWindow(object):
    """One window: the face of a batch loop of B = 1 (``batch``) without the window dimension (``TimeAwarePatchLoop``)."""
    graphed = False
    last_run_mode = "native"

    def _face(self, batch) -> None:
        self.batch = b = batch
        self.theta, self.d_theta, self.exp_avg, self.exp_avg_sq, self.losses = b.theta[0], b.d_theta[0], b.exp_avg[0], b.exp_avg_sq[0], b.losses[0]

    def __getattr__(self, name):                       # (only what the face does not hold itself: step, voxel, iwe, affine, ...)
        if name == "batch":
            raise AttributeError(name)
        return getattr(self.batch, name)

    t, owner_bwd = (property(lambda self, k=k: getattr(self.batch, k), lambda self, v, k=k: setattr(self.batch, k, v)) for k in ("t", "owner_bwd"))

    def run(self, n_iter: int) -> torch.Tensor:
        """``n_iter`` more iterations, enqueued by one C call; returns their losses [n_iter] (device)."""
        return self.batch.run(n_iter)[0]

    def value_and_grad(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loss [0-d], d loss / d theta [2, gh, gw]) at ``theta`` through the same kernels, without the Adam step -- for optimisers
        that live on the host (scipy)."""
        loss, grad = self.batch.value_and_grad(theta[None])
        return loss[0], grad[0]


class TimeAwareMultiReferencePatchLoop(_OneWindow):
    """One window at K reference times: the face of a ``TimeAwareMultiReferencePatchLoopBatch`` of B = 1."""

    def __init__(self, plan: EventPlan, patch_size: Tuple[int, int], sliding_window: Tuple[int, int], theta0: torch.Tensor,
                 time_aware: dict, w_variance: float = 1.0, w_flow_norm: float = 0.0, w_image_gradient: float = 0.0,
                 omit_boundary: bool = False, pad: int = 0, halo="auto", lr: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 capacity: int = 1024, theta_mask: Optional[torch.Tensor] = None):
        self.plan = plan
        self._face(TimeAwareMultiReferencePatchLoopBatch([plan], patch_size, sliding_window, theta0[None], time_aware, w_variance,
                                                         w_flow_norm, w_image_gradient, omit_boundary, pad, halo, lr, betas, eps, capacity,
                                                         theta_mask))


class TimeAwarePatchLoop(_OneWindow):
    """One window: the face of a ``TimeAwarePatchLoopBatch`` of B = 1 (``batch``) without the window dimension.  ``theta0`` and the
    state ``theta`` / ``d_theta`` / ``exp_avg`` / ``exp_avg_sq`` are [2, gh, gw], ``theta_mask`` [gh, gw], ``losses`` [capacity]: views
    of the batch's buffers, so writing into them writes what the kernels read.  Every other attribute is the batch's."""

    def __init__(self, plan: EventPlan, patch_size: Tuple[int, int], sliding_window: Tuple[int, int], theta0: torch.Tensor,
                 time_aware: dict, w_variance: float = 1.0, w_flow_norm: float = 0.0, w_image_gradient: float = 0.0,
                 omit_boundary: bool = False, pad: int = 0, halo="auto", lr: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 capacity: int = 1024, theta_mask: Optional[torch.Tensor] = None, owner_bwd: Optional[bool] = None):
        self.plan = plan
        self._face(TimeAwarePatchLoopBatch([plan], patch_size, sliding_window, theta0[None], time_aware, w_variance, w_flow_norm,
                                           w_image_gradient, omit_boundary, pad, halo, lr, betas, eps, capacity, theta_mask, owner_bwd))
