"""The Adam loop of the multi-reference patch-flow contrast maximisation (the solver's ``multi_reference`` block with
``native: true``) as one C call, without autograd (kernels: csrc/cmax_multiref.hip, csrc/iwe_multiref_slab.hip).

    loss(theta) = -(w / (K N)) sum_k var(IWE_k(dense(theta))) + w_n flow_norm(dense) + w_g image_gradient(dense)

One iteration, on buffers allocated once per loop -- 7 launches, 8 with a regulariser weight, whatever K is:

    ebos_upsample_patch_flow_f32             theta [2, gh, gw] -> dense [2, H, W]
    ebos_iwe_dense_slab_multiref_f32         accumulate over (work item, k) + combine over (pixel block, k): K IWEs, K variances, moments
    ebos_flow_regularisers_f32               (with a regulariser weight) value partials + gradient image
    ebos_iwe_dense_tiled_multiref_bwd_f32    -> d_dense: the sum over the references inside each tile, + the regularisers' gradient
    (fold)                                   sum_k variance_k -> the one scalar the Adam step kernel reads
    ebos_upsample_patch_flow_bwd_adam_f32    -> d_theta, the Adam step of every grid element, loss[it]

The family: the variance contrast alone, optional ``flow_norm`` / ``image_gradient``, no ``iwe.blur_sigma``, a plan tile and halo that
``_hip.slab_multiref_configs()`` lists; anything else belongs to the autograd loop of ``ContrastMaximization``.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _hip
from .._hip import check, ptr, stream_ptr
from ..event_plan import EventPlan, _refuse_deferred, multi_reference_shifts, multiref_slab_halo


class MultiReferencePatchLoop(object):
    """Constructor shape of ``time_aware_loop.TimeAwarePatchLoop`` with ``directions`` (1 to 4 reference times) and ``norm`` (N of
    the block's ``normalize``; 1 without it) in place of the time-aware block."""
    graphed = False
    last_run_mode = "native"

    def __init__(self, plan: EventPlan, patch_size: Tuple[int, int], sliding_window: Tuple[int, int], theta0: torch.Tensor,
                 directions, w_variance: float = 1.0, w_flow_norm: float = 0.0, w_image_gradient: float = 0.0,
                 omit_boundary: bool = False, pad: int = 0, halo="auto", lr: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 capacity: int = 1024, theta_mask: Optional[torch.Tensor] = None, norm: float = 1.0, splits: Optional[int] = None):
        shifts = multi_reference_shifts(plan, directions)   # (ValueError: no normalised time / no reference fraction / bad directions)
        if not plan.binned:
            raise NotImplementedError("MultiReferencePatchLoop walks the runs of a binned plan: build it with a tile")
        _refuse_deferred(plan, "MultiReferencePatchLoop")
        self.halo = multiref_slab_halo(plan.tile, halo)     # (NotImplementedError names the built triples)
        if float(w_variance) == 0.0:
            raise ValueError("w_variance must be non-zero")
        norm = float(norm)
        if norm != norm or norm == 0.0 or norm in (float("inf"), float("-inf")):
            raise ValueError(f"norm must be finite and non-zero, got {norm}")
        self.lib = lib = _hip.require_gpu()
        self.plan, self.patch, self.slide = plan, tuple(int(v) for v in patch_size), tuple(int(v) for v in sliding_window)
        self.shifts, self.K, self.norm = tuple(shifts), len(shifts), norm
        self.w_var, self.w_norm, self.w_tv = float(w_variance), float(w_flow_norm), float(w_image_gradient)
        self.omit, self.pad = bool(omit_boundary), (int(pad), int(pad))
        self.splits = max(1, plan.resolve_splits(splits))
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        dev = plan.device
        H, W = plan.image_size
        K = self.K
        f32 = dict(dtype=torch.float32, device=dev)
        self.theta = theta0.detach().to(**f32).contiguous().clone()
        _, self.gh, self.gw = self.theta.shape
        self.theta_mask = None if theta_mask is None else theta_mask.detach().to(**f32).reshape(self.gh, self.gw).contiguous()
        self.d_theta = torch.empty_like(self.theta)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t = 0
        self.has_reg = self.w_norm != 0.0 or self.w_tv != 0.0
        self.dense, self.d_dense = torch.empty((2, H, W), **f32), torch.empty((2, H, W), **f32)
        self.d_reg = torch.empty((2, H, W), **f32) if self.has_reg else None
        self.iwes = torch.empty((K, H + 2 * self.pad[0], W + 2 * self.pad[1]), **f32)
        self.variances = torch.empty(K, **f32)
        self.contrast = torch.empty(1, **f32)                  # sum_k variance_k
        self.moments = torch.empty((K, 2), dtype=torch.float64, device=dev)
        # loss = scale * sum_k variance_k + regularisers (from the float32 weight the C side reads: the same scalar on both sides)
        self.scale = -ctypes.c_float(self.w_var).value / (K * self.norm)
        self.upstream = torch.full((1,), self.scale, **f32)
        nbytes = int(lib.ebos_iwe_slab_multiref_workspace_bytes(K, H, W, plan.tile[0], plan.tile[1], self.halo, self.splits, self.pad[0],
                                                                self.pad[1]))
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=dev)   # zero-filled once
        self.n_reg = int(lib.ebos_flow_regularisers_partials()) if self.has_reg else 0
        self.reg_partials = torch.zeros(max(self.n_reg, 1), dtype=torch.float64, device=dev)
        self.scratch_up = torch.empty(int(lib.ebos_upsample_bwd_scratch_bytes(self.gh, W)) // 4, **f32)
        self.losses = torch.zeros(max(int(capacity), 1), **f32)

    def problem(self) -> "_hip.CmaxMultirefProblem":
        """The loop's buffers as the ``ebos_cmax_multiref_problem`` struct of the C ABI."""
        plan = self.plan
        q = _hip.CmaxMultirefProblem()
        q.xs, q.ys, q.dts, q.key_offsets, q.n = ptr(plan.x), ptr(plan.y), ptr(plan.dt), ptr(plan.key_offsets), plan.n
        q.H, q.W = plan.image_size
        q.tile_h, q.tile_w, q.halo = plan.tile[0], plan.tile[1], self.halo
        q.pad_h, q.pad_w, q.omit_boundary, q.splits = self.pad[0], self.pad[1], int(self.omit), self.splits
        q.K = self.K
        for k, s in enumerate(self.shifts):
            q.shifts[k] = s
        q.gh, q.gw, (q.patch_h, q.patch_w), (q.slide_h, q.slide_w) = self.gh, self.gw, self.patch, self.slide
        q.w_variance, q.w_flow_norm, q.w_image_gradient, q.norm = self.w_var, self.w_norm, self.w_tv, self.norm
        q.lr, q.beta1, q.beta2, q.eps = self.lr, self.betas[0], self.betas[1], self.eps
        q.theta, q.d_theta, q.exp_avg, q.exp_avg_sq = ptr(self.theta), ptr(self.d_theta), ptr(self.exp_avg), ptr(self.exp_avg_sq)
        q.step, q.steps_done = ptr(self.step), self.t
        q.dense, q.d_dense, q.d_reg = ptr(self.dense), ptr(self.d_dense), ptr(self.d_reg)
        q.iwes, q.variances, q.contrast, q.moments, q.upstream = ptr(self.iwes), ptr(self.variances), ptr(self.contrast), ptr(self.moments), ptr(self.upstream)
        q.workspace, q.workspace_bytes = ptr(self.workspace), self.workspace.numel()
        q.reg_partials, q.upsample_scratch, q.upsample_scratch_bytes = ptr(self.reg_partials), ptr(self.scratch_up), 4 * self.scratch_up.numel()
        q.losses, q.losses_cap, q.theta_mask = ptr(self.losses), self.losses.numel(), ptr(self.theta_mask)
        return q

    def solve(self, n_iter: int) -> torch.Tensor:
        """``n_iter`` more iterations, enqueued by one C call; returns their losses [n_iter] (device).  A second call continues the
        first: the Adam state and the step count stay on the loop."""
        n_iter = int(n_iter)
        if self.t + n_iter > self.losses.numel():
            raise ValueError(f"capacity {self.losses.numel()} < {self.t} steps done + {n_iter}")
        t0 = self.t
        with _hip.on_device(self.plan.device):
            check(self.lib.ebos_cmax_multiref_solve_f32(ctypes.byref(self.problem()), n_iter, stream_ptr()), "ebos_cmax_multiref_solve")
        self.t += n_iter
        return self.losses[t0:t0 + n_iter]

    run = solve

    def value_and_grad(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loss [0-d], d loss / d theta [2, gh, gw]) at ``theta`` through the same kernels, without the Adam step -- for optimisers
        that live on the host (scipy)."""
        with _hip.on_device(self.plan.device):
            self.theta.copy_(theta.detach().to(self.theta))
            check(self.lib.ebos_cmax_multiref_gradient_f32(ctypes.byref(self.problem()), stream_ptr()), "ebos_cmax_multiref_gradient")
            loss = self.scale * self.contrast[0]
            if self.n_reg:
                loss = loss + self.reg_partials.sum().to(torch.float32)
        return loss, (self.d_theta.clone() if self.theta_mask is None else self.d_theta * self.theta_mask)
