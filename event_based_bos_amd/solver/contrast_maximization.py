"""``ContrastMaximization`` -- the solver the reference's release references but does not ship
(configs/README.md:65 points at a missing src/solver/contrast_maximization.py).

objective(theta) = - contrast(IWE(warp(events, motion(theta)))) [+ weighted regularisers on the flow]

    motion_model "dense-flow"      theta = patch-flow grid [2, gh, gw] (``patch.size`` / ``patch.sliding_window``),
                                   upsampled to a dense flow (src/solver/patch_eklt.py:173-204), optimised with Adam
                                   (loop shape of src/solver/generative_max_likelihood.py:306-341)
    motion_model "2d-translation"  theta = (trans_x, trans_y); exhaustive grid sweep over ``parameters`` min/max
                                   (the optuna "uniform"/grid sampler, :238-255), optionally refined with Adam

Everything per event runs in the fused tile-private HIP pipeline on an ``EventPlan`` built once per window.
YAML keys read (same names as configs/hot_plate1.yaml:46-80 of the reference): warp_direction, motion_model,
parameters, cost, cost_with_weight, outer_padding, iwe.{method, blur_sigma}, patch.{size, sliding_window, pyramid.{coarsest, finest}},
optimizer.{method (Adam | CG | BFGS | L-BFGS-B | TNC | SLSQP | Newton-CG | trust-ncg | trust-krylov | grid | random | TPE | optuna + sampler),
sampler, seed, n_iter, parameters.lr, options, graph, fused,
refine_iters}.

``optimizer.method: Newton-CG | trust-ncg | trust-krylov`` (``SCIPY_HESSP_METHODS``; dense-flow on the plain warp only): scipy's
second-order methods, the ``hessp`` of the reference's ``scipy_autograd.minimize`` (src/solver/scipy_autograd/scipy_minimize.py:106-107).
Value, gradient and Hessian-vector product of the contrast come from ``EventPlan.contrast_dense_hvp`` -- explicit operators, no
double backward --, through the patch-grid upsampling, its transpose and the event-thresholding mask; ``flow_norm`` /
``image_gradient`` add torch's double backward of their own expressions.  Pyramid scales, masks, ``outer_padding``, ``iwe.blur_sigma``,
both contrast costs with weights, ``optimizer.options`` and the warm start work as for the first-order scipy methods.  Such a solver
builds its plan with ``emit="full"`` and, without an explicit ``tile``, on (64, 64); ``fused``, ``resident`` and graph capture are
off, ``loop_mode`` reports "hessp", ``hessp_calls`` counts the products of the last estimate.  With a 2-DoF motion model,
``time_aware`` or ``multi_reference`` the constructor raises ``NotImplementedError`` naming ``optimizer.method``; so it does for a
``tile`` / ``halo`` whose two LDS windows are float32 (``tile: [32, 64]``, ``halo: 32`` on (64, 64)): their sums do not repeat their
bits and two estimates of one window would differ (``_check_hessp_tile``).  Not covered:
``dogleg`` / ``trust-exact`` (full Hessians) and ``trust-constr`` (the solver has no bounds or constraints to give it).

``time_aware: {time_bin, scheme: upwind | burgers, t0_location: first | middle, clamp}`` (optional, this build's; dense-flow only): the
time-aware objective.  The dense flow is the flow at t0; ``flow_voxel_batch`` transports it into ``time_bin`` bins, every event is
warped by the flow of its own bin (``EventPlan.contrast_voxel``) and the gradient comes back through the voxel's adjoint to the
patch grid.  Such a solver runs the autograd loop (Adam or the scipy methods): ``fused``, ``resident`` and HIP-graph capture are off
and ``loop_mode`` reports "autograd".  Without the block nothing changes.

``time_aware.native: true`` (default false) runs the same objective as a fixed pipeline of HIP kernels instead
(``solver/time_aware_loop.py``: one C call enqueues the whole Adam loop, the scipy methods evaluate value and gradient through it, at
every pyramid scale): ``loop_mode`` reports "native", ``fused`` is True, ``history`` comes from the loop's losses, and without an
explicit ``tile`` the plan takes a built tile of the time-aware forward kernel, (64, 64).  Its family is the variance contrast alone
with optional ``flow_norm`` / ``image_gradient``, no ``iwe.blur_sigma``, Adam or a scipy method; the constructor raises
``NotImplementedError`` naming the key that leaves it.

``time_aware.directions: [...]`` (optional; 1 to 4 of ``'first' | 'middle' | 'last' | 'before' | 'after' | float``) scores the
time-aware flow at several reference times and averages the contrasts, ``time_aware.normalize: true`` (default false, needs
``directions``) divides each by cost c of the window's zero-flow IWE (1 where that is 0):

    loss(theta) = -(1/K) sum_k sum_c w_c C_c(blur(IWE_k(voxel(dense(theta))))) / N_c + regularisers

``t0_location`` says where the base flow lives in the voxel and does not depend on the reference times.  Without ``native`` this is
the autograd loop through ``EventPlan.contrast_voxel_multi`` / ``iwe_voxel_multi``; with ``native: true`` the loop of
``time_aware_loop.TimeAwareMultiReferencePatchLoopBatch`` (``ebos_cmax_voxel_multiref_solve_batch_f32``), in the same family and
with the same batch methods as ``native`` alone.  Without ``directions`` nothing changes.

``multi_reference: {directions: [...], normalize: false, fused: null}`` (optional, this build's; dense-flow only): the multi-reference
focus objective against event collapse.  The same flow is scored at 1 to 4 reference times (``'first' | 'middle' | 'last' | 'before' |
'after' | float``) and the contrasts are averaged:

    loss(theta) = -(1/K) sum_k sum_c w_c C_c(blur(IWE_k)) / N_c + regularisers

``normalize: true`` sets N_c to cost c of the window's zero-flow IWE (once per window, without gradient; 1 where that is 0), else
N_c = 1.  ``fused`` is ``EventPlan.iwe_dense_multi``'s.  Such a solver runs the autograd loop (Adam or the scipy methods; ``fused``,
``resident`` and graph capture are off, ``loop_mode`` reports "autograd"), builds its plan with ``emit="full"`` and, without an
explicit ``tile``, on (64, 64).  Together with ``time_aware`` or a 2-DoF motion model the constructor raises ``NotImplementedError``.

``multi_reference.native: true`` (default false) runs the same objective as a fixed pipeline of HIP kernels instead
(``solver/multi_reference_loop.py``: the K-image slab forward, the K-reference tile-private backward, one C call for the whole Adam
loop; the scipy methods evaluate value and gradient through it, at every pyramid scale): ``loop_mode`` reports "native", ``fused`` is
True and ``history`` comes from the loop's losses.  Its family is the variance contrast alone with optional ``flow_norm`` /
``image_gradient``, no ``iwe.blur_sigma``, ``outer_padding`` 0, Adam or a scipy method, and a ``tile`` / ``halo`` that
``_hip.slab_multiref_configs()`` lists (``halo: auto`` takes the tile's default built halo); the constructor raises
``NotImplementedError`` naming the key that leaves it.
"""
from __future__ import annotations

import logging
from typing import Callable, Dict, List, NamedTuple, Optional

import numpy as np
import torch

from .. import _hip, costs, ops
from ..flow_voxel import flow_voxel_batch
from .._staging import to_gpu
from ..event_image_converter import EventImageConverter
from ..event_plan import EventPlan, TimeAwarePlanStack, canonical_runs, multi_reference_fractions
from . import fused_loop, multi_reference_loop, time_aware_loop
from .base import SolverBase

logger = logging.getLogger(__name__)

CONTRAST_COSTS = ("image_variance", "gradient_magnitude")
SCIPY_METHODS = ("CG", "BFGS", "L-BFGS-B", "TNC", "SLSQP")  # first-order methods of scipy.optimize.minimize
# second-order methods of scipy.optimize.minimize that take a Hessian-vector product (``hessp``): plain dense-flow warp only
SCIPY_HESSP_METHODS = ("Newton-CG", "trust-ncg", "trust-krylov")


def parse_time_aware(block) -> Optional[dict]:
    """The ``time_aware`` block of the solver's configuration -> {time_bin, scheme, t0_location, clamp}, plus ``native``,
    ``directions`` and ``normalize`` where the block gives them (absent means false / one reference time, the plan's own), or None
    without one."""
    if block is None:
        return None
    block = dict(block)
    unknown = sorted(set(block) - {"time_bin", "scheme", "t0_location", "clamp", "native", "directions", "normalize"})
    if unknown:
        raise ValueError(f"time_aware: unknown key(s) {unknown}; it takes time_bin, scheme, t0_location, clamp, native, directions, "
                         "normalize")
    if "time_bin" not in block:
        raise ValueError("time_aware needs time_bin, the number of bins of the flow voxel")
    out = {"time_bin": ops.check_time_bins(block["time_bin"]), "scheme": block.get("scheme", "upwind"),
           "t0_location": block.get("t0_location", "middle"), "clamp": None if block.get("clamp") is None else float(block["clamp"])}
    if "native" in block:   # (returned as given; a block without the key parses to what it always did, and means false)
        if not isinstance(block["native"], bool):
            raise ValueError(f"time_aware.native must be true or false, got {block['native']!r}")
        out["native"] = block["native"]
    if out["scheme"] not in ("upwind", "burgers"):
        raise ValueError(f"time_aware.scheme must be 'upwind' or 'burgers', got {out['scheme']!r}")
    if out["t0_location"] not in ("first", "middle"):
        raise ValueError(f"time_aware.t0_location must be 'first' or 'middle', got {out['t0_location']!r}")
    if "directions" in block:   # (the reference times the voxel is scored at; returned only where given, like native)
        directions = block["directions"]
        if isinstance(directions, (list, tuple)):
            directions = [float(d) if isinstance(d, (int, float)) and not isinstance(d, bool) else d for d in directions]
        multi_reference_fractions(directions)   # (ValueError for 'random', an empty list, more than four, an unknown name)
        out["directions"] = list(directions)
    if "normalize" in block:
        if not isinstance(block["normalize"], bool):
            raise ValueError(f"time_aware.normalize must be true or false, got {block['normalize']!r}")
        if "directions" not in block:
            raise ValueError("time_aware.normalize belongs to the multi-reference objective: it needs time_aware.directions")
        out["normalize"] = block["normalize"]
    return out


MULTI_REFERENCE_TILE = (64, 64)   # halo 16 keeps up to four windows of it in the LDS (ebos_iwe_multiref_fits)


def parse_multi_reference(block) -> Optional[dict]:
    """The ``multi_reference`` block of the solver's configuration -> {directions, normalize, fused}, plus ``native`` where the block
    gives it (absent means false), or None without one."""
    if block is None:
        return None
    block = dict(block)
    unknown = sorted(set(block) - {"directions", "normalize", "fused", "native"})
    if unknown:
        raise ValueError(f"multi_reference: unknown key(s) {unknown}; it takes directions, normalize, fused, native")
    if "directions" not in block:
        raise ValueError("multi_reference needs directions, the reference times the flow is scored at")
    directions = block["directions"]
    if isinstance(directions, (list, tuple)):
        directions = [float(d) if isinstance(d, (int, float)) and not isinstance(d, bool) else d for d in directions]
    multi_reference_fractions(directions)   # (ValueError for 'random', an empty list, more than four, an unknown name)
    normalize, fused = block.get("normalize", False), block.get("fused", None)
    if not isinstance(normalize, bool):
        raise ValueError(f"multi_reference.normalize must be true or false, got {normalize!r}")
    if fused is not None and not isinstance(fused, bool):
        raise ValueError(f"multi_reference.fused must be true, false or null, got {fused!r}")
    out = {"directions": list(directions), "normalize": normalize, "fused": fused}
    if "native" in block:   # (returned as given; a block without the key parses to what it always did, and means false)
        if not isinstance(block["native"], bool):
            raise ValueError(f"multi_reference.native must be true or false, got {block['native']!r}")
        out["native"] = block["native"]
    return out


class _Warp(NamedTuple):
    """How the solver's dense flow becomes the image(s) whose contrast it maximises (``_resolve_warp``)."""
    operand: Callable    # flow [2, H, W] -> what the plan operators take: the flow itself, or its flow voxel [T, 2, H, W]
    images: Callable     # (plan, operand) -> image [h, w] or images [K, h, w]: the blurred objective's operator
    contrast: Callable   # (plan, operand, cost) -> the fused raw contrast (0-d; the mean over the references where there are several)
    mean: bool           # do the cost kernels on ``images`` give one value per reference, to be averaged?
    norms: Callable      # plan -> {cost: N_c}: all 1.0 where the block has no ``normalize``


def patch_grid_shape(image_size, patch_size, sliding_window):
    """Number of patch centres per axis (src/solver/patch_eklt.py:85-89)."""
    gh = len(np.arange(0, image_size[0] - patch_size[0] + sliding_window[0], sliding_window[0]))
    gw = len(np.arange(0, image_size[1] - patch_size[1] + sliding_window[1], sliding_window[1]))
    return gh, gw


class ContrastMaximizationMixin(object):
    """The CMax logic, independent of WHICH ``SolverBase`` it is composed over (``make_solver_class``): the build's
    own (``solver/base.py``) or the reference's (``src/solver/base.py:54-378``, whose visualisation / flow-error methods the
    driver calls, bos_event.py:202-219).  Needs from the base's constructor only ``slv_config`` and ``orig_image_shape``
    (both bases set them, reference :72-83); everything else it uses is set up by ``_cmax_setup``."""

    def _cmax_setup(self) -> None:
        cfg = self.slv_config = dict(self.slv_config or {})
        self.orig_image_shape = tuple(int(v) for v in self.orig_image_shape)
        # attributes the build's SolverBase provides and the reference's does not (it calls the padding ``padding``, :74-76)
        if not hasattr(self, "pad"):
            self.pad = int(cfg.get("outer_padding", 0))
        if not hasattr(self, "warp_direction"):
            self.warp_direction = cfg.get("warp_direction", "first")
        if not hasattr(self, "motion_model"):  # (the reference's visualize_one_batch_warp reads self.motion_model, :183)
            self.motion_model = cfg.get("motion_model", "dense-flow")
        if not hasattr(self, "previous_best"):
            self.previous_best = None
        self.cost_with_weight: Dict[str, float] = dict(cfg.get("cost_with_weight") or {cfg.get("cost", "image_variance"): 1.0})
        self.contrast_terms = {k: w for k, w in self.cost_with_weight.items() if k in CONTRAST_COSTS}
        self.flow_terms = {k: w for k, w in self.cost_with_weight.items() if k not in CONTRAST_COSTS}
        if not self.contrast_terms:
            raise ValueError(f"cost_with_weight needs at least one contrast cost of {CONTRAST_COSTS}")
        unknown = [k for k in self.flow_terms if k not in costs.functions]
        if unknown:
            raise KeyError(f"unknown cost(s) {unknown}; registered: {sorted(costs.functions)}")
        self.flow_cost = (costs.HybridCost("minimize", self.flow_terms) if self.flow_terms else None)
        self.omit_boundary = bool(cfg.get("omit_boundary", False))
        iwe_cfg = cfg.get("iwe") or {}
        if iwe_cfg.get("method", "bilinear_vote") != "bilinear_vote":
            raise NotImplementedError("the contrast objective is defined on method='bilinear_vote'")
        # iwe.blur_sigma > 0: the contrast is taken on create_iwe(events, sigma=blur_sigma) of the tensor branch
        # (3-tap blur, src/event_image_converter.py:399-404).  It removes the spurious optimum at zero flow that
        # integer sensor coordinates create (un-warped events hit single pixels, any sub-pixel warp spreads them).
        self.blur_sigma = float(iwe_cfg.get("blur_sigma", 0) or 0)
        pcfg = cfg.get("patch") or {}
        self.patch_size = tuple(pcfg.get("size", (24, 32)))
        self.sliding_window = tuple(pcfg.get("sliding_window", self.patch_size))
        self.pyramid = pcfg.get("pyramid") or None
        # patch.do_event_thresholding / patch.event_thres (src/solver/patch_eklt.py:62-67): a patch is estimated only
        # when more than event_thres events fall inside it (:118-126); the others keep zero flow
        self.do_event_thresholding = bool(pcfg.get("do_event_thresholding", False))
        self.event_thres = int(pcfg.get("event_thres", 0) or 0)
        if self.pyramid and not (int(self.pyramid["coarsest"]) >= int(self.pyramid["finest"]) >= 1):
            raise ValueError("patch.pyramid needs coarsest >= finest >= 1")
        ocfg = cfg.get("optimizer") or {}
        self.opt_method = ocfg.get("method", "Adam")
        # Newton-CG / trust-ncg / trust-krylov (module docstring): scipy with the contrast's Hessian-vector product
        self.hessp = self.opt_method in SCIPY_HESSP_METHODS
        self.hessp_calls = 0   # products of the last estimate
        self.n_iter = int(ocfg.get("n_iter", 100))
        self.lr = float((ocfg.get("parameters") or {}).get("lr", 0.05))
        self.scipy_options = dict(ocfg.get("options") or {})
        self.refine_iters = int(ocfg.get("refine_iters", 0))  # 2-DoF models: Adam steps after the grid sweep
        # optimizer.sampler (configs/hot_plate1.yaml:69, src/solver/generative_max_likelihood.py:215-226): the outer loop of
        # method "optuna" -- grid / uniform, random, TPE; optimizer.seed (this build's) makes random / TPE draws reproducible
        self.sampler = ocfg.get("sampler", "grid")
        self.sampler_seed = ocfg.get("seed", None)
        self.param_ranges = cfg.get("parameters") or {}  # {name: {min, max}} or the reference's list of names (_param_range)
        # solver.halo: "auto" (default) = run-time LDS windows per tile (event_plan.resolve_halo: each work item sizes its window
        # from a bound on its own displacements; BOS flows are a few pixels), bounded by the largest built halo; an integer
        # = that built halo for every tile.  Either way displacements beyond a window are handled exactly (spill path).
        self.halo = "auto" if cfg.get("halo", "auto") == "auto" else int(cfg.get("halo"))
        # `tile` (optional, [rows, cols]): the source tile of the window plans instead of the one that fills the GPU best with ONE
        # window -- a recording's windows are independent, and larger tiles let more of them run side by side (WindowPipeline)
        self.tile = tuple(int(v) for v in cfg["tile"]) if cfg.get("tile") else None
        # optimizer.graph: capture one whole iteration (upsample -> fused objective -> backward -> Adam update) into a
        # HIP graph and replay it.  Measured on MI355X / ROCm 7.2 (tools/bench_solver.py, 2 M events at 1280x720):
        # 0.195 ms per replayed iteration against 0.68 ms for the eager loop (interpreter + autograd overhead around
        # ~0.1 ms of GPU work); capture + instantiation cost 1-8 ms, i.e. ~10 iterations -- on by default, and any
        # capture failure falls back to the eager loop.
        self.use_graph = bool(ocfg.get("graph", True))
        self.graphed = False
        # optimizer.fused (default on): objectives of the family -w var(IWE) + w_n flow_norm + w_g image_gradient run as
        # a fixed pipeline of HIP kernels (solver/fused_loop.py) instead of through autograd
        self.fused_loop = bool(ocfg.get("fused", True))
        self.fused = False
        # optimizer.resident (default: whenever the geometry allows it): the fused loop as ONE resident launch
        # (ebos_cmax_patch_solve_resident_f32: same trajectory bit for bit, 42.8 -> 31.5 us per iteration at 2 M events); False keeps
        # the four launches per iteration.  ``loop_mode`` = what the last fused loop actually ran ("resident" / "pipeline").
        self.resident = ocfg.get("resident", None)
        self.loop_mode: Optional[str] = None
        self.loop_modes: List[str] = []   # ... of every pyramid scale of the last estimate, coarse to fine
        self.history: List[float] = []
        # time_aware (module docstring): the flow is the flow at t0 of a voxel, every event reads its own bin; the autograd loop only
        self.time_aware = parse_time_aware(cfg.get("time_aware"))
        if self.time_aware is not None:
            if self.motion_model != "dense-flow":
                raise NotImplementedError(f"time_aware is defined for motion_model 'dense-flow', not {self.motion_model!r}")
            self.use_graph = self.fused_loop = False
            self.resident = False
            if self.time_aware.get("native", False):
                self._check_native("time_aware", "the variance contrast alone")
        # multi_reference (module docstring): the contrast is the mean over several reference times; the autograd loop only
        self.multi_reference = parse_multi_reference(cfg.get("multi_reference"))
        if self.multi_reference is not None:
            if self.time_aware is not None:
                raise NotImplementedError("multi_reference together with time_aware: the multi_reference block is defined on the "
                                          "plain dense-flow warp; to score the time-aware flow at several reference times, put "
                                          "`directions` (and `normalize`) into the time_aware block and drop multi_reference")
            if self.motion_model != "dense-flow":
                raise NotImplementedError(f"multi_reference is defined for motion_model 'dense-flow', not {self.motion_model!r}")
            self.use_graph = self.fused_loop = False
            self.resident = False
            if self.multi_reference.get("native", False):
                self._check_native_multi_reference()
        if self.hessp:
            if self.motion_model != "dense-flow" or self.time_aware is not None or self.multi_reference is not None:
                raise NotImplementedError(f"optimizer.method {self.opt_method!r}: the Hessian-vector product is defined for motion_model "
                                          "'dense-flow' on the plain warp (no time_aware or multi_reference block); there, Adam or one "
                                          f"of {SCIPY_METHODS}")
            self.use_graph = self.fused_loop = False
            self.resident = False
            self._check_hessp_tile()
        self._warp = self._resolve_warp()

    def _check_native(self, block: str, variance_alone: str, before_method=None, last=None) -> None:
        """``<block>.native``: the family of the block's native loop (``time_aware_loop.TimeAwarePatchLoop`` /
        ``multi_reference_loop.MultiReferencePatchLoop``), or NotImplementedError naming the key outside it.  ``variance_alone``: the
        block's wording of the contrast clause; ``before_method`` / ``last``: the block's own clauses (-> what, or None), in their place
        among the shared ones -- the first clause that fails is the one reported."""
        what = None
        if set(self.contrast_terms) != {"image_variance"}:
            what = f"cost / cost_with_weight: the contrast {sorted(self.contrast_terms)} ({variance_alone})"
        elif not set(self.flow_terms) <= set(fused_loop.FLOW_TERMS):
            what = f"cost_with_weight: {sorted(set(self.flow_terms) - set(fused_loop.FLOW_TERMS))} (flow_norm and image_gradient only)"
        elif self.blur_sigma > 0:
            what = f"iwe.blur_sigma: {self.blur_sigma} (the un-blurred IWE only)"
        else:
            what = before_method() if before_method is not None else None
            if what is None and self.opt_method != "Adam" and self.opt_method not in SCIPY_METHODS:
                what = f"optimizer.method: {self.opt_method!r} (Adam or one of {SCIPY_METHODS})"
            if what is None and last is not None:
                what = last()
        if what is not None:
            raise NotImplementedError(f"{block}.native does not cover " + what + "; drop native to run the autograd loop")

    def _check_hessp_tile(self) -> None:
        """The ``SCIPY_HESSP_METHODS`` need a loss and a gradient that repeat their bits: scipy's Newton iterations carry a last bit
        through the kinks of the vote (**Bits**).  ``contrast_dense_hvp`` gives that where the two LDS windows of its
        first call are float64; as float32 windows they are summed by LDS float atomics in the order the hardware picks -- on tile
        (32, 64) the gradient repeated its bits in 0 of 10 calls and two estimates of one window ended 1.9e-6 px apart after four
        iterations (tests/test_gpu_hvp_tiles.py).  Such a (tile, halo) is refused here, at construction, with the tiles that work; a
        tile without a built halo raises ``hvp_tile_halo``'s NotImplementedError."""
        from .. import _hip
        from ..event_plan import hvp_float64_tiles, hvp_tile_halo

        try:
            _hip.load_library()
        except _hip.HipUnavailableError:
            return   # nothing to ask yet: the first estimate raises this error itself
        tile = tuple(int(v) for v in self.plan_tile())
        halo, kind = hvp_tile_halo(tile, self.halo, 2, f"optimizer.method {self.opt_method!r}")
        if kind != 2:
            raise NotImplementedError(
                f"optimizer.method {self.opt_method!r} with tile {list(tile)}, halo {self.halo!r}: the IWE and the tangent image of one "
                f"product would be float32 LDS windows (halo {halo}; ebos_iwe_multiref_fits), whose sums do not repeat their bits, "
                "and the second-order methods amplify a last bit: two estimates of one window would differ.  Tiles whose two "
                f"windows are float64 with halo \"auto\": {[list(t) for t in hvp_float64_tiles()]}; without a `tile` key the "
                f"solver plans on {list(MULTI_REFERENCE_TILE)}")

    def _check_native_multi_reference(self) -> None:
        """``multi_reference.native``: the shared clauses, no ``outer_padding``, a (tile, halo) the K-image kernels are built for."""
        from ..event_plan import multiref_slab_halo

        def tile_halo():
            try:
                multiref_slab_halo(self.plan_tile(), self.halo)
            except NotImplementedError as e:
                return f"tile / halo: {e}"

        self._check_native("multi_reference", "the variance contrast alone, no gradient_magnitude",
                           lambda: f"outer_padding: {self.pad} (0 only)" if self.pad != 0 else None, tile_halo)

    # ------------------------------------------------------------------ objective pieces
    def _zero_flow_norms(self, plan: EventPlan, normalize: bool, attr: str, zero_flow_iwe) -> Dict[str, float]:
        """N_c of a loss over several reference times: cost c of the window's zero-flow IWE ``zero_flow_iwe(plan)`` (the same image at
        every reference time), blurred like the objective's; once per plan (kept on it as ``attr``), without gradient, 1 where the
        value is 0 -- or all 1 without ``normalize``."""
        if not normalize:
            return {name: 1.0 for name in self.contrast_terms}
        key = (self.pad, self.blur_sigma, self.omit_boundary, tuple(self.contrast_terms))
        cached = plan.__dict__.get(attr)
        if cached is None or cached[0] != key:
            with torch.no_grad():
                iwe = zero_flow_iwe(plan)
                if self.blur_sigma > 0:
                    iwe = EventImageConverter._gaussian_blur3(iwe, self.blur_sigma)
                vals = {name: float((ops.image_variance if name == "image_variance" else ops.gradient_magnitude)(iwe, self.omit_boundary))
                        for name in self.contrast_terms}
            cached = plan.__dict__[attr] = (key, {k: (v if v != 0.0 else 1.0) for k, v in vals.items()})
        return cached[1]

    def _zero_flow_iwe_dense(self, plan: EventPlan) -> torch.Tensor:
        H, W = plan.image_size
        zero = torch.zeros((2, H, W), dtype=torch.float32, device=plan.device)
        return plan.iwe_dense_multi(zero, [0.0 if plan.ref_fraction is None else float(plan.ref_fraction)],
                                    pad=(self.pad, self.pad), halo=self.halo, fused=False)[0]

    def _zero_flow_iwe_voxel(self, plan: EventPlan) -> torch.Tensor:
        H, W = plan.image_size   # (the same image for every voxel bin, too)
        zero = torch.zeros((self.time_aware["time_bin"], 2, H, W), dtype=torch.float32, device=plan.device)
        return plan.iwe_voxel(zero, pad=(self.pad, self.pad), halo=self.halo)

    def _multi_reference_norms(self, plan: EventPlan) -> Dict[str, float]:
        return self._zero_flow_norms(plan, self.multi_reference["normalize"], "_multiref_norms", self._zero_flow_iwe_dense)

    def _time_aware_norms(self, plan: EventPlan) -> Dict[str, float]:
        return self._zero_flow_norms(plan, self.time_aware.get("normalize", False), "_time_aware_norms", self._zero_flow_iwe_voxel)

    def _resolve_warp(self) -> "_Warp":
        """The solver's warp, from ``multi_reference`` / ``time_aware`` (the geometry keys are read at call time)."""
        kw = lambda: {"pad": (self.pad, self.pad), "halo": self.halo}   # noqa: E731
        ta, mr = self.time_aware, self.multi_reference
        ones = lambda plan: {name: 1.0 for name in self.contrast_terms}   # noqa: E731
        to_voxel = None if ta is None else \
            (lambda flow: flow_voxel_batch(flow[None], ta["time_bin"], ta["scheme"], ta["t0_location"], ta["clamp"])[0])
        if mr is not None:
            return _Warp(lambda flow: flow,
                         lambda plan, x: plan.iwe_dense_multi(x, mr["directions"], fused=mr["fused"], **kw()),
                         lambda plan, x, cost: plan.contrast_dense_multi(x, mr["directions"], cost, self.omit_boundary, fused=mr["fused"], **kw()),
                         True, self._multi_reference_norms)
        if ta is not None and ta.get("directions") is not None:
            return _Warp(to_voxel,
                         lambda plan, x: plan.iwe_voxel_multi(x, ta["directions"], **kw()),
                         lambda plan, x, cost: plan.contrast_voxel_multi(x, ta["directions"], cost, self.omit_boundary, **kw()),
                         True, self._time_aware_norms)
        if ta is not None:
            return _Warp(to_voxel,
                         lambda plan, x: plan.iwe_voxel(x, **kw()),
                         lambda plan, x, cost: plan.contrast_voxel(x, cost, self.omit_boundary, **kw()),
                         False, ones)
        return _Warp(lambda flow: flow,
                     lambda plan, x: plan.iwe_dense(x, **kw()),
                     lambda plan, x, cost: plan.contrast_dense(x, cost, self.omit_boundary, **kw()),
                     False, ones)

    def _contrast(self, plan: EventPlan, flow: torch.Tensor) -> torch.Tensor:
        warp = self._warp
        x = warp.operand(flow)
        norms = warp.norms(plan)
        if self.blur_sigma > 0:
            images = EventImageConverter._gaussian_blur3(warp.images(plan, x), self.blur_sigma)
        total = 0.0
        for name, wgt in self.contrast_terms.items():
            if self.blur_sigma > 0:   # the cost kernels on the blurred image(s); the fused operators take the un-blurred ones only
                value = (ops.image_variance if name == "image_variance" else ops.gradient_magnitude)(images, self.omit_boundary)
                if warp.mean:
                    value = value.mean()
            else:
                value = warp.contrast(plan, x, name)
            total = total + (wgt / norms[name]) * value   # (a warp without norms has all 1.0, and wgt / 1.0 == wgt exactly)
        return total

    def objective(self, plan: EventPlan, flow: torch.Tensor) -> torch.Tensor:
        """Loss to MINIMISE: -contrast + regularisers (weights from cost_with_weight)."""
        loss = -self._contrast(plan, flow)
        if self.flow_cost is not None:
            ones = torch.ones(flow.shape[-2:], dtype=flow.dtype, device=flow.device)
            loss = loss + self.flow_cost.calculate({"flow": flow, "omit_boundary": self.omit_boundary, "weights": ones})
        return loss

    # ------------------------------------------------------------------ estimate
    def estimate(self, events, *args, **kwargs) -> np.ndarray:
        """events [n, 4] (x=row, y=col, t, p) -> flow [2, H, W] (numpy), like the reference's solvers."""
        plan = self._build_plan(events)
        self._fractional_stream = plan.fractional
        self.history = []
        # The optimisation loops below call loss.backward() thousands of times on graphs of one or two nodes: with the autograd
        # engine's device thread each call pays two thread hand-offs (~35 us of a ~100 us iteration, tools/bench_autograd.py);
        # single-threaded, backward runs on the calling thread.  Restored on exit.
        with torch.autograd.set_multithreading_enabled(False):
            if self.motion_model == "dense-flow":
                flow = self._estimate_patch_flow(plan)
            elif self.motion_model in ("2d-translation", "rigid-optical-flow"):
                theta = self._estimate_translation(plan)
                H, W = self.orig_image_shape
                flow = (-theta).reshape(2, 1, 1).expand(2, H, W)  # dense flow equivalent of theta (src/warp.py:186-187)
            else:
                raise NotImplementedError(f"motion_model {self.motion_model!r}")
        return flow.detach().cpu().numpy().astype(np.float64)

    def _build_plan(self, events) -> EventPlan:
        """The plan of one window, in the emit the solver's warp reads."""
        ev = to_gpu(events)
        # (the objective uses unit weights: the lean build -- compact events + offsets only -- is all it reads; windows with
        # fractional, i.e. undistorted, coordinates fall back to the full build inside)
        # (a stream of sub-pixel rectified events is fractional window after window: once a window fell back, the lean
        # attempt -- its kernels and its read-back, ~0.3 ms of a 100 k-event window's build -- is skipped until a full build finds
        # integer coordinates again; either build is valid for either kind of window)
        if self.multi_reference is not None:   # the shifted reference times read the SoA events of the full build
            return EventPlan.build(ev, self.orig_image_shape, self.warp_direction, True, tile=self.plan_tile(), emit="full")
        if self.time_aware is not None:   # the bins travel with the SoA events of the full build
            return EventPlan.build(ev, self.orig_image_shape, self.warp_direction, True, tile=self.plan_tile(), emit="full",
                                   time_bin=self.time_aware["time_bin"])
        if self.hessp:   # the second-order kernels read the SoA events of the full build; the owner kernel adds in run order, and
            # Newton's iterations amplify a last bit: every run in a canonical order, so two builds of a window give the same solve
            return canonical_runs(EventPlan.build(ev, self.orig_image_shape, self.warp_direction, True, tile=self.plan_tile(), emit="full"))
        return EventPlan.build(ev, self.orig_image_shape, self.warp_direction, True, tile=self.plan_tile(),
                               emit="full" if getattr(self, "_fractional_stream", False) else "compact")

    def _native_batch(self) -> bool:
        """Does ``estimate_batch`` solve several windows per launch?  The ``time_aware: {native: true}`` family with Adam."""
        return (self.time_aware is not None and bool(self.time_aware.get("native", False)) and self.opt_method == "Adam"
                and self.motion_model == "dense-flow")

    def estimate_batch(self, windows, max_batch: int = 8) -> np.ndarray:
        """``estimate`` for several windows of a recording: float64 [len(windows), 2, H, W].  A ``time_aware: {native: true}``
        configuration with ``optimizer.method: Adam`` solves the windows in chunks of ``max_batch`` through
        ``time_aware_loop.TimeAwarePatchLoopBatch`` (one Adam iteration of a chunk in the launches of one window), at every pyramid
        scale; the coarse-to-fine initialisation and ``patch_mask`` are each window's own and ``_warm_start()`` is the common start.
        Every other configuration is the loop of ``estimate``.  Per window: ``histories[b]`` and ``patch_flows[b]``; ``loop_modes`` per
        pyramid scale; ``history`` and ``patch_flow`` hold the last window's.  A window ``estimate`` refuses is refused the same way."""
        windows = list(windows)
        flows = self._estimate_chunks(len(windows), max_batch, lambda b: windows[b],
                                      lambda lo, hi: [self._build_plan(ev) for ev in windows[lo:hi]])
        return np.zeros((0, 2) + self.orig_image_shape, dtype=np.float64) if flows is None else flows.cpu().numpy()

    def estimate_batch_prepared(self, prepared, frames=None, background=None, max_batch: int = 8, device_out: bool = False):
        """``estimate_batch`` on ``evaluation.PreparedWindows`` that carry their raw columns (the signature of the generative
        solvers' method; ``frames`` and ``background`` are not read): float64 [B, 2, H, W], numpy or -- ``device_out`` -- a device
        tensor.  A ``time_aware: {native: true}`` configuration with Adam turns chunks of ``max_batch`` windows into a stacked plan
        straight from the columns (``TimeAwarePlanStack.from_raw``: no float64 event array, one read-back per chunk) and solves them
        through the batch loop; every other configuration is ``estimate`` on ``prepared.events(b)``, window by window.  Sets
        ``histories``, ``patch_flows``, ``loop_modes``, ``history`` and ``patch_flow`` as ``estimate_batch`` does."""
        if getattr(prepared, "cols", None) is None or getattr(prepared, "ranges", None) is None:
            raise ValueError("estimate_batch_prepared needs windows that carry their raw columns (evaluation.window_ingest_raw_batch)")
        ranges, dev = list(prepared.ranges), prepared.cols[2].device
        flows = self._estimate_chunks(len(ranges), max_batch, prepared.events, lambda lo, hi: TimeAwarePlanStack.from_raw(
            prepared.cols, ranges[lo:hi], self.orig_image_shape, self.warp_direction, self.plan_tile(), self.time_aware["time_bin"],
            roi=prepared.roi, remove=prepared.remove, ticks_per_second=prepared.ticks_per_second))
        if flows is None:
            flows = torch.zeros((0, 2) + self.orig_image_shape, dtype=torch.float64, device=dev)
        return flows.to(dev) if device_out else flows.cpu().numpy()

    def _estimate_chunks(self, n: int, max_batch: int, events_of, plans_of) -> Optional[torch.Tensor]:
        """The windows 0 .. n - 1 of ``estimate_batch`` / ``estimate_batch_prepared``: float64 [n, 2, H, W] (a host tensor from the
        window-by-window loop, a device tensor from the batch loop), or None for no window.  ``events_of(b)``: the events of window b
        for ``estimate``; ``plans_of(lo, hi)``: the plans, or the ready plan stack, of the chunk of windows lo .. hi - 1."""
        max_batch = int(max_batch)
        if max_batch < 1:
            raise ValueError(f"max_batch must be at least 1, got {max_batch}")
        self.histories, self.patch_flows = [], []
        if n == 0:
            return None
        if not self._native_batch():
            flows = []
            for b in range(n):
                flows.append(self.estimate(events_of(b)))
                self.histories.append(list(self.history))
                self.patch_flows.append(getattr(self, "patch_flow", None))
            return torch.from_numpy(np.stack(flows).astype(np.float64))
        max_batch = min(max_batch, _hip.CMAX_VOXEL_MAX_BATCH)
        flows = [self._estimate_patch_flow_batch(plans_of(c0, min(c0 + max_batch, n))) for c0 in range(0, n, max_batch)]
        self.history, self.patch_flow = self.histories[-1], self.patch_flows[-1]
        return torch.cat(flows).detach().to(torch.float64)

    def _estimate_patch_flow_batch(self, plans) -> torch.Tensor:
        """``_estimate_patch_flow`` for one chunk of windows through the batch loop: [B, 2, H, W] (device).  ``plans``: binned
        time-aware plans of one geometry, or their ready ``TimeAwarePlanStack``."""
        H, W = self.orig_image_shape
        stack = plans if isinstance(plans, TimeAwarePlanStack) else EventPlan.stack_time_aware(plans)
        plans = stack.plans
        B, dev = len(plans), stack.device
        histories = [[] for _ in plans]
        self.loop_modes, per_scale = [], []
        theta = None
        for patch_size, sliding_window, n_iter in self.pyramid_scales():
            masks = [self.patch_mask(plan, patch_size, sliding_window) for plan in plans]
            mask = None if masks[0] is None else torch.stack(masks)
            init = self._scale_start(theta, B, patch_size, sliding_window, mask, dev)   # (every window from its own coarser scale)
            loop = self._native_time_aware_loop(stack, patch_size, sliding_window, init, n_iter, mask)
            loop.run(n_iter)
            self.graphed, self.fused, self.loop_mode = False, True, loop.last_run_mode
            self.loop_modes.append(loop.last_run_mode)
            for b, row in enumerate(loop.losses[:, :n_iter].cpu().tolist()):   # (one read-back per scale)
                histories[b] += row
            theta = loop.theta
            per_scale.append(theta)
        self.histories += histories
        self.patch_flows += [theta[b] for b in range(B)]
        self.patch_flow_per_scale = [t[B - 1] for t in per_scale]
        self.patch_size_used, self.sliding_window_used = patch_size, sliding_window
        return torch.stack([ops.upsample_patch_flow(theta[b], patch_size, sliding_window, (H, W)) for b in range(B)])

    def _warm_start(self):
        """Warm start handed over by ``set_previous_frame_best_estimation`` -- the build's base stores it as
        ``previous_best``, the reference's as ``previous_frame_best_estimation`` (src/solver/base.py:355-361)."""
        prev = getattr(self, "previous_best", None)
        return prev if prev is not None else getattr(self, "previous_frame_best_estimation", None)

    def plan_tile(self):
        """Source tile of the window plans: the configuration built for this solver's ``halo`` that fills the GPU best
        (``halo: 16`` -- windows whose displacements stay within ~16 px -- selects the smaller LDS windows)."""
        from ..event_plan import choose_tile

        if self.tile is not None:
            return self.tile
        if self.multi_reference is not None or self.hessp:   # (the two windows of the tangent pass fit like two references)
            return MULTI_REFERENCE_TILE
        if self.time_aware is not None and self.time_aware.get("native", False):
            # the native loop's forward is the tiled time-aware kernel: a tile it is built for with this halo, (64, 64) first
            from .. import _hip

            halo = 32 if self.halo == "auto" else self.halo
            built = [(th, tw) for th, tw, hl in _hip.tiled_configs() if hl == halo]
            if built:
                return time_aware_loop.DEFAULT_TILE if time_aware_loop.DEFAULT_TILE in built else built[0]
        return choose_tile(self.orig_image_shape, 32 if self.halo == "auto" else self.halo)

    def pyramid_scales(self):
        """[(patch_size, sliding_window, n_iter)] coarse to fine.  Without ``patch.pyramid`` one scale (``patch.size``);
        with ``patch.pyramid: {coarsest: c, finest: f}`` the square patches c, c/2, ... of
        src/solver/patch_eklt_pyramid2.py:55-83 (scales 1 .. int(log2(c / f)) + 1, slide = patch) and its
        iteration split ``n_iter // (finest_scale - scale + 1)`` (:260)."""
        if not self.pyramid:
            return [(self.patch_size, self.sliding_window, self.n_iter)]
        c, f = int(self.pyramid["coarsest"]), int(self.pyramid["finest"])
        finest_scale = int(np.log2(c / f)) + 2
        out = []
        for i in range(1, finest_scale):
            size = (c // (2 ** (i - 1)),) * 2
            out.append((size, size, max(1, self.n_iter // (finest_scale - i + 1))))
        return out

    def patch_mask(self, plan: EventPlan, patch_size, sliding_window) -> Optional[torch.Tensor]:
        """[gh, gw] float32 on the device: 1 where the patch holds more than ``event_thres`` events, else 0 -- or None
        when thresholding is off.  The reference crops the whole event array once per patch
        (src/solver/patch_eklt.py:118-126); here the counts are box sums over the plan's per-pixel histogram
        (``EventPlan.patch_event_counts``), without a host read-back."""
        if not self.do_event_thresholding:
            return None
        return (plan.patch_event_counts(patch_size, sliding_window) > self.event_thres).to(torch.float32)

    def _scale_start(self, coarser: Optional[torch.Tensor], B: int, patch_size, sliding_window, mask: Optional[torch.Tensor],
                     device: torch.device) -> torch.Tensor:
        """The start [B, 2, gh, gw] of one pyramid scale for B windows: each window's patch flow of the coarser scale (``coarser``
        [B, 2, gh', gw']) resized -- resize(x0, patch_image_size), pyramid2.py:253-255 --, at the coarsest scale the common warm
        start or zeros; then ``mask`` [B, gh, gw] (patches that are not estimated start, and stay, at zero)."""
        gh, gw = patch_grid_shape(self.orig_image_shape, patch_size, sliding_window)
        if coarser is not None:
            init = torch.nn.functional.interpolate(coarser, size=(gh, gw), mode="bilinear", align_corners=False)
        elif self._warm_start() is not None:
            init = to_gpu(self._warm_start(), device=device, dtype=torch.float32).reshape(1, 2, gh, gw).expand(B, 2, gh, gw).contiguous()
        else:
            init = torch.zeros((B, 2, gh, gw), dtype=torch.float32, device=device)
        return init if mask is None else init * mask[:, None]

    def _native_time_aware_loop(self, plans, patch_size, sliding_window, theta: torch.Tensor, capacity: int, mask: Optional[torch.Tensor]):
        """The ``time_aware.native`` loop of one pyramid scale: of one plan, or of a ``TimeAwarePlanStack`` (the batch classes), at
        one reference time or at the block's ``directions``."""
        batch, multi = isinstance(plans, TimeAwarePlanStack), self.time_aware.get("directions") is not None
        loop_cls = {(False, False): time_aware_loop.TimeAwarePatchLoop, (False, True): time_aware_loop.TimeAwareMultiReferencePatchLoop,
                    (True, False): time_aware_loop.TimeAwarePatchLoopBatch,
                    (True, True): time_aware_loop.TimeAwareMultiReferencePatchLoopBatch}[(batch, multi)]
        return loop_cls(plans, patch_size, sliding_window, theta, self.time_aware, self.contrast_terms["image_variance"],
                        self.flow_terms.get("flow_norm", 0.0), self.flow_terms.get("image_gradient", 0.0), self.omit_boundary, self.pad,
                        self.halo, self.lr, capacity=capacity, theta_mask=mask)

    def _estimate_patch_flow(self, plan: EventPlan) -> torch.Tensor:
        H, W = self.orig_image_shape
        self.history, self.patch_flow_per_scale, self.loop_modes = [], [], []
        self.hessp_calls = 0
        theta = None
        for patch_size, sliding_window, n_iter in self.pyramid_scales():
            mask = self.patch_mask(plan, patch_size, sliding_window)
            init = self._scale_start(None if theta is None else theta[None], 1, patch_size, sliding_window,
                                     None if mask is None else mask[None], plan.device)[0]
            theta = self._optimise_patch_grid(plan, init.clone(), patch_size, sliding_window, n_iter, mask)
            self.patch_flow_per_scale.append(theta)
        self.patch_flow = theta
        self.patch_size_used, self.sliding_window_used = patch_size, sliding_window
        return ops.upsample_patch_flow(theta, patch_size, sliding_window, (H, W))

    def _optimise_patch_grid(self, plan: EventPlan, theta: torch.Tensor, patch_size, sliding_window, n_iter: int,
                             mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        H, W = self.orig_image_shape
        capacity = n_iter if self.opt_method == "Adam" else 1   # (of a native block's loop: a scipy method records no losses there)
        if self.time_aware is not None and self.time_aware.get("native", False):
            loop = self._native_time_aware_loop(plan, patch_size, sliding_window, theta.detach(), capacity, mask)
            return self._optimise_native(loop, theta, n_iter)
        if self.multi_reference is not None and self.multi_reference.get("native", False):
            norm = self._multi_reference_norms(plan)["image_variance"]
            loop = multi_reference_loop.MultiReferencePatchLoop(plan, patch_size, sliding_window, theta.detach(), self.multi_reference["directions"],
                                                                self.contrast_terms["image_variance"], self.flow_terms.get("flow_norm", 0.0),
                                                                self.flow_terms.get("image_gradient", 0.0), self.omit_boundary, self.pad,
                                                                self.halo, self.lr, capacity=capacity, theta_mask=mask, norm=norm)
            return self._optimise_native(loop, theta, n_iter)
        if self.hessp:
            value_and_grad, hessp = self._hessp_objective(plan, patch_size, sliding_window, mask)
            self.graphed, self.fused, self.loop_mode = False, False, "hessp"
            self.loop_modes.append("hessp")
            return self._run_scipy(None, theta.detach(), n_iter, value_and_grad=value_and_grad, hessp=hessp)
        theta = theta.requires_grad_(True)

        def evaluate():  # (mask: the gradient of a patch that is not estimated is zero, so it keeps its masked start)
            dense = ops.upsample_patch_flow(theta if mask is None else theta * mask, patch_size, sliding_window, (H, W))
            return self.objective(plan, dense)

        if self.fused_loop and fused_loop.supported(self.contrast_terms, self.flow_terms, self.blur_sigma, self.opt_method,
                                                    plan, self.halo, sliding_window):
            theta_start = theta.detach().clone()   # (a torn resident launch leaves the loop's state partly written: start over from here)

            def make_loop():
                return fused_loop.FusedPatchLoop(plan, patch_size, sliding_window, theta_start.clone(), self.contrast_terms.get("image_variance", 0.0),
                                                 self.flow_terms.get("flow_norm", 0.0), self.flow_terms.get("image_gradient", 0.0),
                                                 self.omit_boundary, self.pad, self.halo, self.lr, capacity=n_iter,
                                                 w_gradient_magnitude=self.contrast_terms.get("gradient_magnitude", 0.0), theta_mask=mask,
                                                 blur_sigma=self.blur_sigma)

            loop = fused_loop.run_rebuilding_torn(make_loop, n_iter, self.resident)
            self.graphed, self.fused, self.loop_mode = loop.graphed, True, loop.last_run_mode
            self.loop_modes.append(loop.last_run_mode)  # (per pyramid scale, coarse to fine)
            self.history += loop.losses[:n_iter].cpu().tolist()   # (one conversion: 600 float() calls cost 0.1 ms of a 12 ms window)
            return loop.theta
        self.fused = False
        if self.time_aware is not None or self.multi_reference is not None:
            self.loop_mode = "autograd"
            self.loop_modes.append("autograd")
        if self.opt_method in SCIPY_METHODS:
            if self.fused_loop and fused_loop.objective_supported(self.contrast_terms, self.flow_terms, self.blur_sigma, plan,
                                                                  self.halo):
                loop = fused_loop.FusedPatchLoop(plan, patch_size, sliding_window, theta, self.contrast_terms.get("image_variance", 0.0),
                                                 self.flow_terms.get("flow_norm", 0.0), self.flow_terms.get("image_gradient", 0.0),
                                                 self.omit_boundary, self.pad, self.halo, self.lr, capacity=1,
                                                 w_gradient_magnitude=self.contrast_terms.get("gradient_magnitude", 0.0), theta_mask=mask)
                self.fused = True
                return self._run_scipy(None, theta, n_iter, value_and_grad=loop.value_and_grad)
            return self._run_scipy(evaluate, theta, n_iter)
        if self.opt_method != "Adam":
            raise NotImplementedError(f"optimizer.method {self.opt_method!r}: Adam or one of {SCIPY_METHODS}")

        def iteration(opt):
            opt.zero_grad(set_to_none=True)
            loss = evaluate()
            loss.backward()
            opt.step()
            return loss.detach()

        self.graphed = False
        losses = torch.zeros(max(n_iter, 1), dtype=torch.float32, device=plan.device)
        done = 0
        if self.use_graph and n_iter > 4:
            done = self._run_graphed(iteration, theta, losses, n_iter)
        if not self.graphed:
            opt = torch.optim.Adam([theta], lr=self.lr)
            for it in range(done, n_iter):
                losses[it] = iteration(opt)
        self.history += losses[:n_iter].cpu().tolist()
        return theta.detach()

    def _optimise_native(self, loop, theta: torch.Tensor, n_iter: int) -> torch.Tensor:
        """One pyramid scale of a ``time_aware.native`` / ``multi_reference.native`` solve on the block's loop: the Adam loop as one C
        call, or a scipy method on the loop's ``value_and_grad``."""
        self.graphed, self.fused, self.loop_mode = False, True, loop.last_run_mode
        self.loop_modes.append(loop.last_run_mode)
        if self.opt_method != "Adam":
            return self._run_scipy(None, theta.detach(), n_iter, value_and_grad=loop.value_and_grad)
        loop.run(n_iter)
        self.history += loop.losses[:n_iter].cpu().tolist()
        return loop.theta

    def _hessp_objective(self, plan: EventPlan, patch_size, sliding_window, mask: Optional[torch.Tensor]):
        """(value_and_grad, hessp) of one pyramid scale for the ``SCIPY_HESSP_METHODS``, without an autograd graph through the events:

            loss(theta) = -sum_c w_c C_c(dense) + regularisers(dense),   dense = U (m * theta)
            H_theta p   = m * U^T (H_dense (U (m * p)))

        with U the patch-grid upsampling (linear; U^T is its backward kernel) and m the event-thresholding mask.  The contrast's
        value, gradient and product come from ``EventPlan.contrast_dense_hvp``, whose ``state`` -- what depends on the flow alone --
        is kept from the last ``value_and_grad`` and reused by every ``hessp`` at that theta (scipy asks for many products per outer
        iteration); a product asked at another theta evaluates there first.  The regularisers are plain torch expressions on the
        dense flow: their product is torch's double backward of the same expressions, on the device."""
        H, W = self.orig_image_shape
        grid = patch_grid_shape((H, W), patch_size, sliding_window)
        kw = {"cost": dict(self.contrast_terms), "omit_boundary": self.omit_boundary, "blur_sigma": self.blur_sigma,
              "pad": (self.pad, self.pad), "halo": self.halo}
        zero = torch.zeros((2, H, W), dtype=torch.float32, device=plan.device)
        kept = {"theta": None, "dense": None, "state": None}

        def to_dense(t):
            t = t.to(device=plan.device, dtype=torch.float32)
            return ops.upsample_patch_flow(t if mask is None else t * mask, patch_size, sliding_window, (H, W))

        def to_grid(d):
            g = ops.upsample_patch_flow_adjoint(d, grid, patch_size, sliding_window)
            return g if mask is None else g * mask

        def regularisers(dense, v=None):
            """(value, gradient, product with v or None) of the flow terms at ``dense``."""
            f = dense.detach().requires_grad_(True)
            with torch.enable_grad():
                ones = torch.ones(f.shape[-2:], dtype=f.dtype, device=f.device)
                r = self.flow_cost.calculate({"flow": f, "omit_boundary": self.omit_boundary, "weights": ones})
                (g,) = torch.autograd.grad(r, f, create_graph=v is not None)
                hv = None
                if v is not None:   # (a term that is piecewise linear in the flow, like the total variation, has no curvature)
                    hv = torch.autograd.grad(g, f, v, allow_unused=True)[0] if g.requires_grad else None
                    hv = torch.zeros_like(f) if hv is None else hv
            return r.detach(), g.detach(), hv

        def value_and_grad(theta):
            dense = to_dense(theta)
            value, d_flow, _, state = plan.contrast_dense_hvp(dense, zero, **kw)
            kept["theta"], kept["dense"], kept["state"] = theta.detach().clone(), dense, state
            loss, d_dense = -value, -d_flow
            if self.flow_cost is not None:
                r, g, _ = regularisers(dense)
                loss, d_dense = loss + r, d_dense + g
            return loss, to_grid(d_dense)

        def hessp(theta, p):
            if kept["theta"] is None or not torch.equal(kept["theta"], theta):
                value_and_grad(theta)
            v = to_dense(p)
            hv = -plan.contrast_dense_hvp(kept["dense"], v, state=kept["state"], **kw)[2]
            if self.flow_cost is not None:
                hv = hv + regularisers(kept["dense"], v)[2]
            self.hessp_calls += 1
            return to_grid(hv)

        return value_and_grad, hessp

    def _run_scipy(self, evaluate, theta: torch.Tensor, n_iter: int, value_and_grad=None, hessp=None) -> torch.Tensor:
        """Gradient-based scipy optimisers on the GPU objective, the role of the reference's
        ``scipy_autograd.minimize`` (src/solver/scipy_autograd/scipy_minimize.py:6-125): scipy drives float64 numpy
        parameters on the host; every function/gradient evaluation is one fused forward + backward on the device.
        Line searches need a differentiable start: with integer sensor coordinates the all-zero flow sits on the kink
        of the bilinear vote (every event exactly on a pixel centre), so warm-start these methods
        (``set_previous_frame_best_estimation``) or use Adam, which does not care.  ``hessp(theta, p)``: the Hessian-vector product
        scipy's Newton-CG / trust-region methods ask for (:106-107 of the reference's wrapper), handed on as ``hessp``."""
        import scipy.optimize as sopt

        shape = tuple(theta.shape)
        second = {}
        if hessp is not None:
            second["hessp"] = lambda x, p: hessp(torch.from_numpy(x.reshape(shape)), torch.from_numpy(p.reshape(shape))) \
                .double().cpu().numpy().reshape(-1)

        def fun(x):
            if value_and_grad is not None:  # fixed kernel pipeline, no autograd graph
                loss, grad = value_and_grad(torch.from_numpy(x.reshape(shape)))
                self.history.append(float(loss))
                return self.history[-1], grad.double().cpu().numpy().reshape(-1)
            with torch.no_grad():
                theta.copy_(torch.from_numpy(x.reshape(shape)).to(theta))
            theta.grad = None
            loss = evaluate()
            loss.backward()
            self.history.append(float(loss.detach()))
            return self.history[-1], theta.grad.detach().double().cpu().numpy().reshape(-1)

        x0 = theta.detach().double().cpu().numpy().reshape(-1)
        res = sopt.minimize(fun, x0, jac=True, method=self.opt_method, options={"maxiter": int(n_iter), **self.scipy_options}, **second)
        if not res.success:
            logger.warning(f"Unsuccessful optimization step! ({res.message})")
        self.scipy_result = res
        return torch.from_numpy(res.x.reshape(shape)).to(theta).detach()

    def _run_graphed(self, iteration, theta: torch.Tensor, losses: torch.Tensor, n_iter: int) -> int:
        """Adam loop as a replayed HIP graph.  The first iterations run eagerly on a side stream (they also create
        the plan workspace and Adam state), one iteration is captured, the rest are replays.  Returns the number of
        iterations performed; falls back to the eager loop (self.graphed = False) if capture is not possible."""
        warm = 3
        start = theta.detach().clone()
        try:
            opt = torch.optim.Adam([theta], lr=self.lr, capturable=True)
            side = torch.cuda.Stream(device=theta.device)
            side.wait_stream(torch.cuda.current_stream(theta.device))
            with torch.cuda.stream(side):
                for it in range(warm):
                    losses[it] = iteration(opt)
            torch.cuda.current_stream(theta.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            opt.zero_grad(set_to_none=True)
            # capture_begin/capture_end directly: the torch.cuda.graph() context adds gc.collect() + empty_cache()
            side.wait_stream(torch.cuda.current_stream(theta.device))
            with torch.cuda.stream(side):
                graph.capture_begin()
                try:
                    static_loss = iteration(opt)
                finally:
                    graph.capture_end()
            torch.cuda.current_stream(theta.device).wait_stream(side)
            for it in range(warm, n_iter):  # the capture itself executed nothing: iteration `warm` is the first replay
                graph.replay()
                losses[it] = static_loss
            self.graphed = True
            return n_iter
        except Exception as err:  # capture unsupported for some op: restart the whole loop eagerly
            logger.warning(f"HIP graph capture of the solver iteration failed ({err!r}); running eagerly")
            with torch.no_grad():
                theta.copy_(start)
            theta.grad = None
            self.graphed = False
            return 0

    def _param_range(self, key: str) -> Dict[str, float]:
        """{min, max} of a motion parameter: ``parameters: {trans_x: {min, max}}`` (this solver's YAMLs) or -- when
        ``parameters`` is the reference's LIST of parameter names (configs/hot_plate1.yaml:48-50) -- the sampler ranges of
        ``optimizer.parameters`` (:71-80), default +-30 px."""
        rng = self.param_ranges.get(key) if isinstance(self.param_ranges, dict) else None
        if rng is None:
            rng = ((self.slv_config.get("optimizer") or {}).get("parameters") or {}).get(key)
        return rng if isinstance(rng, dict) and "min" in rng and "max" in rng else {"min": -30.0, "max": 30.0}

    def _translation_loss(self, plan: EventPlan, theta: torch.Tensor) -> torch.Tensor:
        """-contrast of the IWE under the translation ``theta`` [2] (autograd through the 2-DoF tile-private kernels)."""
        iwe = plan.iwe_2dof(theta[None], pad=(self.pad, self.pad), halo=self.halo)[0]
        if self.blur_sigma > 0:
            iwe = EventImageConverter._gaussian_blur3(iwe, self.blur_sigma)
        total = 0.0
        for name, wgt in self.contrast_terms.items():
            fn = ops.image_variance if name == "image_variance" else ops.gradient_magnitude
            total = total + wgt * fn(iwe, self.omit_boundary)
        return -total

    def _translation_loop_fused(self, plan: EventPlan) -> bool:
        """Can the 2-DoF Adam loop run natively (``fused_loop.Fused2dofLoop``: ebos_cmax_2dof_solve_f32)?  The variance contrast
        (optionally of the 3-tap blurred image) on a binned plan -- compact, or the (x, y, dt) format of fractional (undistorted)
        source coordinates -- with a tile-private kernel configuration."""
        from ..event_plan import _slab_ok

        return (self.fused_loop and set(self.contrast_terms) == {"image_variance"} and not self.flow_terms
                and (plan.compact or plan.x is not None) and self.halo is not None and _slab_ok(plan, self.halo) and (not self.blur_sigma or min(plan.image_size) >= 2))

    def _adam_translation(self, plan: EventPlan, theta0: torch.Tensor, n_iter: int) -> torch.Tensor:
        """``n_iter`` Adam steps on (trans_x, trans_y) from ``theta0``: natively when the objective allows it (one C call
        enqueues the whole loop, no host synchronisation per iteration), else through autograd."""
        if self._translation_loop_fused(plan):
            def make_loop():
                return fused_loop.Fused2dofLoop(plan, theta0.detach().clone(), self.contrast_terms["image_variance"], self.omit_boundary, self.pad,
                                                self.halo, self.lr, capacity=max(n_iter, 1), blur_sigma=self.blur_sigma)

            loop = fused_loop.run_rebuilding_torn(make_loop, n_iter, self.resident)   # (the loop works on a copy of theta0)
            self.fused, self.loop_mode = True, loop.last_run_mode
            self.history += loop.losses[:n_iter].cpu().tolist()   # (one conversion: 600 float() calls cost 0.1 ms of a 12 ms window)
            return loop.theta
        self.fused = False
        theta = theta0.clone().requires_grad_(True)
        opt = torch.optim.Adam([theta], lr=self.lr)
        for _ in range(n_iter):
            opt.zero_grad(set_to_none=True)
            loss = self._translation_loss(plan, theta)
            loss.backward()
            opt.step()
            self.history.append(float(loss.detach()))
        return theta.detach()

    def _tpe_translation(self, contrast, rx, ry, batch: int = 32, n_candidates: int = 24, gamma: float = 0.25):
        """``sampler: TPE`` -- a tree-structured Parzen estimator in the shape optuna runs it (src/solver/generative_max_likelihood.py:
        216-219: ``n_startup_trials = max(10, n_iter // 10)`` uniform draws first), batched for the GPU: each round fits the two Parzen
        densities (Gaussian kernels on the best ``gamma`` quantile of the trials so far / on the rest, per parameter, bandwidth from
        the neighbour spacing, plus the uniform prior), draws ``n_candidates`` points per slot from the good density, keeps the one with
        the largest l(x) / g(x), and evaluates ``batch`` such picks as ONE sweep.  optuna itself is not installed here: the algorithm
        follows Bergstra et al. 2011 as optuna documents it, trial for trial it is not optuna's stream (parity unpinned)."""
        rs = np.random.RandomState(self.sampler_seed)
        lo, hi = np.array([rx["min"], ry["min"]], float), np.array([rx["max"], ry["max"]], float)
        n_total = max(1, self.n_iter)
        n_start = min(n_total, max(10, n_total // 10))
        xs = rs.uniform(lo, hi, (n_start, 2))
        vals = contrast(torch.from_numpy(xs.astype(np.float32))).double().cpu().numpy()

        def log_parzen(pts, x):  # [m, 2] kernels (+ the prior) -> log density at x [k, 2], product over the two parameters
            out = np.zeros(len(x))
            for d in range(2):
                mu = np.sort(pts[:, d])
                ext = np.concatenate([[lo[d]], mu, [hi[d]]])
                sig = np.clip(np.maximum(ext[1:-1] - ext[:-2], ext[2:] - ext[1:-1]), (hi[d] - lo[d]) / min(100.0, 1.0 + len(mu)), hi[d] - lo[d])
                mu = np.concatenate([mu, [0.5 * (lo[d] + hi[d])]])
                sig = np.concatenate([sig, [hi[d] - lo[d]]])   # the prior: one wide kernel in the middle of the range
                z = (x[:, d, None] - mu[None]) / sig[None]
                out += np.log(np.mean(np.exp(-0.5 * z * z) / (sig[None] * np.sqrt(2 * np.pi)), axis=1) + 1e-300)
            return out

        while len(xs) < n_total:
            k = min(batch, n_total - len(xs))
            order = np.argsort(-vals)                      # maximise the contrast
            n_good = max(1, int(np.ceil(gamma * len(xs))))
            good, bad = xs[order[:n_good]], xs[order[n_good:]] if len(xs) > n_good else xs
            picks = np.empty((k, 2))
            for j in range(k):
                comp = rs.randint(0, len(good) + 1, n_candidates)            # (index len(good) = the prior)
                spread = np.maximum((hi - lo) / max(4.0, np.sqrt(len(good) + 1.0)), 1e-6)
                centre = np.where((comp == len(good))[:, None], 0.5 * (lo + hi), good[np.minimum(comp, len(good) - 1)])
                width = np.where((comp == len(good))[:, None], hi - lo, spread)
                cand = np.clip(centre + rs.standard_normal((n_candidates, 2)) * width, lo, hi)
                picks[j] = cand[np.argmax(log_parzen(good, cand) - log_parzen(bad, cand))]
            v = contrast(torch.from_numpy(picks.astype(np.float32))).double().cpu().numpy()
            xs, vals = np.concatenate([xs, picks]), np.concatenate([vals, v])
        return torch.from_numpy(xs.astype(np.float32)), torch.from_numpy(vals.astype(np.float32))

    def _estimate_translation(self, plan: EventPlan) -> torch.Tensor:
        """``optimizer.method: grid`` -- exhaustive sweep over the parameter ranges (the optuna grid sampler of
        src/solver/generative_max_likelihood.py:238-255); ``random`` / ``TPE`` (or ``method: optuna`` + ``optimizer.sampler``, :215-226)
        -- n_iter uniform draws / a batched Parzen-estimator search inside the same ranges; each optionally refined by
        ``refine_iters`` Adam steps;
        ``Adam`` -- n_iter Adam steps on (trans_x, trans_y) from the warm start (or zero), the loop shape of :306-341."""
        if self.opt_method == "Adam":
            start = self._warm_start()
            theta0 = (torch.zeros(2, dtype=torch.float32, device=plan.device) if start is None else
                      to_gpu(start, device=plan.device, dtype=torch.float32).reshape(2))
            return self._adam_translation(plan, theta0, self.n_iter)
        # optimizer.method: "optuna" + optimizer.sampler (src/solver/generative_max_likelihood.py:215-226) or the sampler's name as the
        # method: grid / uniform (= sweep), random, TPE
        sampler = self.opt_method
        if sampler == "optuna":
            sampler = self.sampler
        sampler = {"sweep": "grid", "uniform": "grid", "tpe": "TPE"}.get(sampler, sampler)
        if sampler not in ("grid", "random", "TPE"):
            raise NotImplementedError(f"optimizer.method {self.opt_method!r} (sampler {self.sampler!r}) for a 2-DoF motion model: "
                                      "Adam, grid / uniform, random or TPE")
        rx, ry = self._param_range("trans_x"), self._param_range("trans_y")

        def contrast(thetas: torch.Tensor) -> torch.Tensor:  # one batched launch sequence for all hypotheses of a round
            return plan.variance_2dof(thetas.to(plan.device), self.omit_boundary, pad=(self.pad, self.pad), halo=self.halo)

        if sampler == "random":
            # optuna.samplers.RandomSampler (:220-221): n_iter independent uniform draws inside parameters.{min, max}; all of them
            # are independent hypotheses, so they are ONE batched sweep (optimizer.seed makes the draws reproducible)
            rs = np.random.RandomState(self.sampler_seed)
            draws = rs.uniform([rx["min"], ry["min"]], [rx["max"], ry["max"]], (max(1, self.n_iter), 2))
            grid = torch.from_numpy(draws.astype(np.float32))
            var = contrast(grid)
        elif sampler == "TPE":
            grid, var = self._tpe_translation(contrast, rx, ry)
        else:
            n = max(2, int(round(np.sqrt(max(self.n_iter, 4)))))
            gx = torch.arange(n, dtype=torch.float32) * ((rx["max"] - rx["min"]) / n) + rx["min"]  # np.arange(min, max, step), :238-255
            gy = torch.arange(n, dtype=torch.float32) * ((ry["max"] - ry["min"]) / n) + ry["min"]
            grid = torch.stack(torch.meshgrid(gx, gy, indexing="ij"), -1).reshape(-1, 2)
            var = contrast(grid)
        grid = grid.to(plan.device)
        self.history = [float(-v) for v in var.cpu()]
        self.sweep_grid, self.sweep_contrast = grid, var
        theta = grid[int(torch.argmax(var).item())]
        if self.refine_iters > 0:  # optimizer.refine_iters: Adam from the best grid point (gradient of the 2-DoF kernels)
            theta = self._adam_translation(plan, theta, self.refine_iters)
        return theta


def make_solver_class(base, name: str = "ContrastMaximization"):
    """``ContrastMaximization`` composed over ``base`` (a ``SolverBase``): constructor signature of the plugin surface
    (src/solver/base.py:64-71), ``estimate`` and the objective from the mixin, everything else -- ``preprocess``, the
    imagers / warpers, and with the reference's base its ``visualize_*`` / ``calculate_flow_error`` /
    ``save_flow_error_as_text`` -- from ``base``."""

    def __init__(self, orig_image_shape, crop_image_shape, calibration_parameter=None, solver_config=None, visualize_module=None):
        base.__init__(self, orig_image_shape, crop_image_shape, {} if calibration_parameter is None else calibration_parameter,
                      {} if solver_config is None else solver_config, visualize_module)
        self._cmax_setup()

    return type(name, (ContrastMaximizationMixin, base), {"__init__": __init__, "__doc__": ContrastMaximizationMixin.__doc__,
                                                          "__module__": __name__})


ContrastMaximization = make_solver_class(SolverBase)


def register_into(solver_module, names=("contrast_maximization", "cmax")):
    """Add the CMax solver to ANOTHER solver registry -- the reference's ``src.solver`` -- built over THAT module's
    ``SolverBase``, so that ``bos_event.py`` drives it unchanged: ``solver.collections[config["solver"]["method"]](...)``
    (bos_event.py:330-337), ``solv.preprocess`` / ``solv.estimate`` (:190-194) and the visualisation / error methods
    (:202-219) all resolve.  Returns the class."""
    cls = make_solver_class(solver_module.SolverBase)
    for n in names:
        solver_module.collections[n] = cls
    return cls
