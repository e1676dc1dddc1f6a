"""The reference's sampled EKLT solvers, ``patch_eklt`` (src/solver/patch_eklt.py) and ``generative_max_likelihood``
(src/solver/generative_max_likelihood.py), as one float64 sweep on the GPU (csrc/eklt_sweep.hip, ``ebos_eklt_*``).

Both are the original EKLT formulation: every patch (``GenerativePatchIndependent`` = the reference's ``PatchEklt``) or the one ROI
(``GenerativeGlobal`` = ``GenerativeMaximumLikelihood``) is scored on its own against the event histogram under a list of hypotheses
(v | angle, optionally a translation p of the model image's gradients), and the best hypothesis wins:

    P0 = v_x T_p(gx) + v_y T_p(gy) on the box (|P0| if no_polarity, * we[box]),  P = P0 / (|P0|_F + 1e-4),
    Q = q[box] / |q[box]|_F,  cost = w_diff_norm max_c sum_r |P - Q|

with T_p cv2.warpPerspective of the whole image by (p_x rows, p_y columns) in OpenCV's classic path (the coordinate rounded to 1/32
pixel, the float32 table weights, the sum in double; restated in tests/_eklt_warp64.py and not pinned against OpenCV, which is absent
where this package is developed).  Per window the prepare pass of the other generative solvers leaves gx, gy, q, we on the device
(``ebos_gml_prepare_batch_f64``), the dependent solver's selection picks the patches (``ebos_gml_dep_select_batch``: centre inside
the crop and, with ``do_event_thresholding``, more than ``event_thres`` events in the box), ``ebos_eklt_sweep_batch_f64`` scores
P boxes x K hypotheses and takes each box's argmin (the lowest index on a tie; a NaN cost never wins), and
``ebos_eklt_patch_flow_batch_f64`` scatters the winners' (v_x, v_y) -- (sin, cos) of the angle model -- into the patch grid and
upsamples it as ``interpolate_dense_flow_from_patch_numpy`` does.  The global solver's flow is its winner, constant over the image.

The sampled route is the reference's only working route of these two solvers (its scipy and torch routes assert the angle model,
then index parameters a one-parameter result does not have, and call a method neither class defines), so ``optimizer.method`` must be
``optuna``; anything else raises ``NotImplementedError``.

Where this departs from the reference:
* ONE hypothesis table per ``estimate`` / ``estimate_batch`` / ``estimate_batch_prepared`` call, shared by all patches and all
  windows of the call.  The reference opens a fresh optuna study per patch; that stream cannot be pinned without optuna, and a
  [P, K, 4] table would not fit.  ``sampler: random``: ``n_iter`` rows, each parameter uniform in [min, max], drawn from numpy's
  global RandomState, trial-major, in the configuration's parameter order.  ``sampler: uniform | grid``: the reference's axes
  ``np.arange(min, max, (max - min) / n_iter)``; with one parameter the axis in order (the whole grid, as the reference visits it),
  with several one ``np.random.randint`` node per axis per trial.  ``sampler: TPE`` raises ``NotImplementedError`` (a sequential
  sampler per patch is outside a one-launch sweep).
* ``PatchEklt._make_measured_increment`` normalises a VIEW of the cached histogram in place when there are no event-hist weights, so
  overlapping patches see each other's division in loop order.  This package always normalises the untouched histogram: identical to
  the reference whenever ``sliding_window == patch_size`` or ``weight_loss_by_event_hist`` is true.
* a box whose histogram norm is 0 is treated as unselected and gets zero flow (the reference divides by zero).
* only ``diff_norm`` may appear in ``cost_with_weight`` (the reference's numpy route hands no flow or pxy to any other term).
* ``run_optuna_config_checks``'s assertions are ``ValueError``s.

``sweep(events, hypotheses, frame=..., background=...) -> (cost [P, K], best_index [P], selected [P])`` scores an explicit
[K, d] table in the configuration's parameterisation (the columns are ``optimizer.parameters`` in order): the brute-force landscape.
After a call ``best_params`` [P, 4] holds the unfolded winners (v_x, v_y, p_x, p_y; 0 where nothing won), ``best_values`` [P] the
winning costs (inf where nothing won), ``estimate_indices`` the patches that were scored; ``best_params_batch``,
``best_values_batch`` and ``estimate_indices_batch`` hold every window of the last ``estimate_batch`` call.  ``estimate`` is a batch
of one; ``estimate_batch`` equals ``estimate`` window by window, bit for bit, when every call draws the same table.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from .. import _hip
from .._hip import check, ptr, stream_ptr
from .._staging import to_gpu
from ..event_image_converter import EventImageConverter
from .base import SolverBase
from .generative import GenerativeMixin, _flag, _History, make_solver_class, register_into
from .generative_dependent import DepAxis

SAMPLERS = ("random", "uniform", "grid")
ROUTES = {None: _hip.EKLT_ROUTE_AUTO, "auto": _hip.EKLT_ROUTE_AUTO, "patch": _hip.EKLT_ROUTE_PATCH, "roi": _hip.EKLT_ROUTE_ROI}


def parameter_keys(gml: dict) -> Tuple[str, ...]:
    """The parameters ``unfold_params`` reads for these options (run_optuna_config_checks)."""
    keys = ("angle",) if _flag(gml, "angle_model") else ("v_x", "v_y")
    if _flag(gml, "optimize_warp"):
        keys += ("p_angle", "p_magn") if _flag(gml, "px-py_as-angle-magnitude") else ("p_x", "p_y")
    return keys


def unfold_table(gml: dict, keys, table) -> np.ndarray:
    """``unfold_params`` over a [K, d] table whose columns are ``keys`` -> [K, 4]: v_x, v_y, p_x, p_y (p = 0 without
    optimize_warp)."""
    t = np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != len(keys) or t.shape[0] < 1:
        raise ValueError(f"EKLT sweep: hypotheses must be [K >= 1, {len(keys)}] ({', '.join(keys)}), got {t.shape}")
    col = {k: t[:, i] for i, k in enumerate(keys)}
    out = np.zeros((t.shape[0], 4), dtype=np.float64)
    if _flag(gml, "angle_model"):
        out[:, 0], out[:, 1] = np.sin(col["angle"]), np.cos(col["angle"])
    else:
        out[:, 0], out[:, 1] = col["v_x"], col["v_y"]
    if _flag(gml, "optimize_warp"):
        if _flag(gml, "px-py_as-angle-magnitude"):
            out[:, 2], out[:, 3] = col["p_magn"] * np.sin(col["p_angle"]), col["p_magn"] * np.cos(col["p_angle"])
        else:
            out[:, 2], out[:, 3] = col["p_x"], col["p_y"]
    return np.ascontiguousarray(out)


def sample_table(opt: dict) -> np.ndarray:
    """The hypothesis table [n_iter, d] of an ``optimizer`` section (see the module's docstring), from numpy's global RandomState."""
    keys = list(opt["parameters"])
    n = int(opt["n_iter"])
    lo = [float(opt["parameters"][k]["min"]) for k in keys]
    hi = [float(opt["parameters"][k]["max"]) for k in keys]
    if opt["sampler"] == "random":
        return np.array([[np.random.uniform(lo[j], hi[j]) for j in range(len(keys))] for _ in range(n)], dtype=np.float64)
    axes = [np.arange(lo[j], hi[j], (hi[j] - lo[j]) / n) for j in range(len(keys))]
    if len(keys) == 1:
        return axes[0].reshape(-1, 1).astype(np.float64)
    return np.array([[axes[j][np.random.randint(len(axes[j]))] for j in range(len(keys))] for _ in range(n)], dtype=np.float64)


class EkltSweepMixin(GenerativeMixin):
    """What the two sampled solvers share: the configuration, the table, the sweep and its records.  A subclass gives the boxes
    (``_eklt_boxes`` [P, 4], ``_eklt_box_bound``), the selection (``_eklt_select``) and the flow (``_eklt_flow``)."""

    _gml_who = "EKLT sweep solver"
    _gml_lists = {"best_params_batch": "best_params", "best_values_batch": "best_values", "estimate_indices_batch": "indices"}

    def _eklt_setup(self) -> None:
        cfg = self.slv_config
        who = self._gml_who
        opt = dict(cfg.get("optimizer") or {})
        gml = dict(cfg.get("generative_ml") or {})
        method = opt.get("method")
        if method != "optuna":
            raise NotImplementedError(f"{who}: optimizer.method {method!r} is not supported (optuna only: the reference's scipy and torch "
                                      "routes of patch_eklt and generative_max_likelihood do not run either)")
        sampler = opt.get("sampler")
        if sampler == "TPE":
            raise NotImplementedError(f"{who}: sampler 'TPE' is not supported (a sequential sampler per patch is outside a one-launch "
                                      f"sweep; use {', '.join(SAMPLERS)})")
        if sampler not in SAMPLERS:
            raise NotImplementedError(f"{who}: sampler {sampler!r} is not supported ({', '.join(SAMPLERS)})")
        params = opt.get("parameters") or {}
        missing = [k for k in parameter_keys(gml) if k not in params]
        if missing:
            raise ValueError(f"{who}: optimizer.parameters lacks {', '.join(missing)} (needed: {', '.join(parameter_keys(gml))})")
        for k, r in params.items():
            if not isinstance(r, dict) or "min" not in r or "max" not in r or not float(r["min"]) <= float(r["max"]):
                raise ValueError(f"{who}: optimizer.parameters.{k} needs min <= max")
        n_iter = int(opt.get("n_iter", 0))
        if n_iter < 1:
            raise ValueError(f"{who}: n_iter {n_iter} < 1")
        cost = dict(cfg.get("cost_with_weight") or {})
        for k, w in cost.items():
            if k != "diff_norm":
                raise NotImplementedError(f"{who}: cost term {k!r} is not supported (diff_norm only: the sampled route hands no flow or "
                                          "pxy to any other term)")
            if isinstance(w, str):
                raise NotImplementedError(f"{who}: cost weight {w!r} of {k} is not supported (numbers only)")
        if "diff_norm" not in cost:
            raise ValueError(f"{who}: cost_with_weight needs diff_norm")
        mi = gml.get("model_image", "current")
        if mi not in ("current", "background"):
            raise ValueError(f"{who}: model_image {mi!r} is not handled by the sampled solvers (current, background)")
        H, W = (int(v) for v in self.orig_image_shape)
        p = (cfg.get("filter") or {}).get("parameters") or {}
        roi = tuple(int(p[k]) for k in ("xmin", "xmax", "ymin", "ymax")) if "filter" in cfg else (0, H, 0, W)
        xmin, xmax, ymin, ymax = roi
        self._gml_roi = (max(0, min(xmin, H)), max(0, min(xmax, H)), max(0, min(ymin, W)), max(0, min(ymax, W)))
        # what GenerativeMixin's driver reads
        self._gml_cfg, self._gml_cost = gml, cost
        self._gml_warp = _flag(gml, "optimize_warp")
        self._gml_n_iter, self._gml_iters = n_iter, []   # no iteration history
        self._gml_velocity = False
        self._gml_n_dim = len(parameter_keys(gml))
        self._gml_frame = None
        self._gml_imager = EventImageConverter((H, W), vote=str((cfg.get("iwe") or {}).get("vote", "atomic")))
        self.cost_func = _History(cost.keys())
        self.iter_cnt = 0
        self.histories = []
        # the sweep's own
        self._eklt_opt = dict(opt, parameters=dict(params))
        self._eklt_keys = tuple(params)
        self._eklt_hyp4 = None        # the table of the call in progress, unfolded [K, 4]
        self._eklt_want_cost = False
        self._eklt_route = None
        self._eklt_dev = {}
        self.best_params = self.best_values = None
        self._eklt_indices = np.zeros(0, dtype=np.int64)
        self.best_params_batch, self.best_values_batch, self.estimate_indices_batch = [], [], []

    @property
    def estimate_indices(self) -> np.ndarray:
        """Indices (row-major over the patch grid; 0 for the global solver's ROI) of the boxes scored in the last window."""
        return self._eklt_indices

    # ------------------------------------------------------------------ the table
    def hypothesis_table(self) -> np.ndarray:
        """Draw the call's table [n_iter, d] in the configuration's parameterisation (numpy's global RandomState)."""
        return sample_table(self._eklt_opt)

    def _gml_run(self, windows, frames, max_batch: int, per_window: bool = True, out_device=None):
        """One table per call, drawn after the argument checks and before the first batch."""
        if len(windows):
            self._eklt_hyp4 = unfold_table(self._gml_cfg, self._eklt_keys, self.hypothesis_table())
        self._eklt_want_cost, self._eklt_route = False, None
        return super()._gml_run(windows, frames, max_batch, per_window, out_device)

    def sweep(self, events, hypotheses, frame=None, background=None, route=None):
        """Score an explicit table: ``hypotheses`` [K, d], the columns being ``optimizer.parameters`` in order ->
        (cost [P, K] float64 -- NaN rows where a box was not scored --, best_index [P] int64 -- -1 there --, selected [P] bool).
        ``route``: None / "auto", or "patch" / "roi" to force one of the kernel's two routes.  Publishes nothing but the kept
        background."""
        if route not in ROUTES:
            raise ValueError(f"{self._gml_who}: route {route!r} is not one of auto, patch, roi")
        hyp4 = unfold_table(self._gml_cfg, self._eklt_keys, hypotheses)
        windows, frames, _ = self._gml_batch_args([events], frame, background, None, single=True)
        self._eklt_hyp4, self._eklt_want_cost, self._eklt_route = hyp4, True, route
        try:
            _, records = self._gml_solve_batch(windows, *self._gml_batch_frames(frames, 0, 1))
        finally:
            self._eklt_want_cost, self._eklt_route = False, None
        r = records[0]
        return r["cost"], r["best_index"], r["best_index"] >= 0

    # ------------------------------------------------------------------ the sweep's part of the batch driver
    def _gml_events(self, windows, prepared: bool, dev):
        if prepared:
            n = len(windows) if self._eklt_needs_events() else 0
            return [windows.events(i).to(dev).reshape(-1, 4).contiguous() for i in range(n)]
        return [to_gpu(ev, device=dev, dtype=torch.float64).reshape(-1, 4).contiguous() for ev in windows]

    def _eklt_needs_events(self) -> bool:
        return False

    def _eklt_canvas(self) -> Tuple[int, int]:
        return (0, 0)

    def _gml_scratch_bytes(self, lib, b: int) -> Tuple[int, int]:
        """The prepare pass's four planes and scalars, or the selection's count canvas: a slice per window."""
        H, W = (int(v) for v in self.orig_image_shape)
        al = lambda n: (n + 255) & ~255
        ch, cw = self._eklt_canvas()
        stride = max(4 * al(H * W * 8) + al(64), al((ch + 1) * (cw + 1) * 4))
        return stride, b * stride

    def _eklt_box_tensor(self, dev):
        key = str(dev)
        if key not in self._eklt_dev:
            self._eklt_dev[key] = torch.from_numpy(np.ascontiguousarray(self._eklt_boxes, dtype=np.int32)).to(dev)
        return self._eklt_dev[key]

    def _gml_solve(self, job):
        lib, b, dev = job.lib, job.b, job.dev
        H, W = (int(v) for v in self.orig_image_shape)
        hyp4 = self._eklt_hyp4
        K, P = int(hyp4.shape[0]), int(self._eklt_boxes.shape[0])
        ph, pw = self._eklt_box_bound
        flags, _, _, _, gx, gy, grad_stride, q, we, _ = job.model
        flags &= _hip.GML_NO_POLARITY | _hip.GML_EVENT_WEIGHTS
        sel = self._eklt_select(job)
        route = ROUTES[self._eklt_route]
        if route == _hip.EKLT_ROUTE_AUTO:
            halo = int(lib.ebos_eklt_sweep_halo(hyp4.ctypes.data, K))
            route = _hip.EKLT_ROUTE_PATCH if lib.ebos_eklt_sweep_fits(ph, pw, halo) else _hip.EKLT_ROUTE_ROI
        nbytes = int(lib.ebos_eklt_sweep_scratch_bytes(b, P, K, route))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cost = torch.full((b, P, K), float("nan"), dtype=torch.float64, device=dev) if self._eklt_want_cost else None
        best_cost = torch.empty(b, P, dtype=torch.float64, device=dev)
        best_index = torch.empty(b, P, dtype=torch.int32, device=dev)
        check(lib.ebos_eklt_sweep_batch_f64(b, H, W, gx, gy, grad_stride, q, we, ptr(self._eklt_box_tensor(dev)), P, ph, pw, ptr(sel),
                                            hyp4.ctypes.data, K, flags, float(self._gml_cost["diff_norm"]), route, ptr(cost),
                                            ptr(best_cost), ptr(best_index), ptr(scratch), nbytes, stream_ptr(dev)),
              "ebos_eklt_sweep_batch_f64")
        hyp_t = torch.from_numpy(hyp4).to(dev)
        self._eklt_flow(job, best_index, hyp_t)
        return cost, best_cost, best_index

    def _gml_records(self, h: np.ndarray, solved) -> List[dict]:
        cost, best_cost, best_index = solved
        hyp4 = self._eklt_hyp4
        bc, bi = best_cost.cpu().numpy(), best_index.cpu().numpy().astype(np.int64)
        cost = None if cost is None else cost.cpu().numpy()
        records = []
        for i in range(len(bi)):
            won = bi[i] >= 0
            params = np.zeros((len(won), 4), dtype=np.float64)
            params[won] = hyp4[bi[i][won]]
            records.append({"history": h[i], "best_params": params, "best_values": bc[i], "indices": np.nonzero(won)[0],
                            "best_index": bi[i], "cost": None if cost is None else cost[i]})
        return records

    def _gml_publish_params(self, record) -> None:
        self.best_params, self.best_values, self._eklt_indices = record["best_params"], record["best_values"], record["indices"]


class GenerativePatchIndependentMixin(EkltSweepMixin):
    """``estimate(events, frame=..., background=...) -> np.ndarray [2, H, W]`` of the reference's PatchEklt (method patch_eklt)."""

    _gml_who = "EKLT patch sweep solver"

    def _patch_setup(self) -> None:
        self._eklt_setup()
        pe = dict(self.slv_config.get("patch_eklt") or {})
        if "patch_size" not in pe:
            raise ValueError(f"{self._gml_who}: patch_eklt.patch_size is required")
        self._dep_patch = int(pe["patch_size"])
        self._dep_slide = int(pe.get("sliding_window", self._dep_patch))
        self._dep_thresholding = bool(pe.get("do_event_thresholding", False))
        thr = pe.get("event_thres")
        if self._dep_thresholding and thr is None:
            raise ValueError(f"{self._gml_who}: do_event_thresholding needs patch_eklt.event_thres")
        self._dep_thres = float(thr) if thr is not None else 0.0
        H, W = (int(v) for v in self.orig_image_shape)
        xmin, xmax, ymin, ymax = self._gml_roi
        rows, cols = DepAxis(H, self._dep_patch, self._dep_slide), DepAxis(W, self._dep_patch, self._dep_slide)
        self.patch_image_size = (rows.g, cols.g)
        self.n_patch = rows.g * cols.g
        self._dep_canvas = (max(int(rows.hi.max()), 0), max(int(cols.hi.max()), 0)) if self._dep_thresholding else (0, 0)
        self._dep_boxes = (rows.boxes(xmin, xmax), cols.boxes(ymin, ymax))
        # a box of the last row or column may pass the image's edge (the grid has ceil((L - p + s) / s) cells): the reference's
        # slices end at the edge
        rhi, chi = np.minimum(rows.hi, H), np.minimum(cols.hi, W)
        self._eklt_boxes = np.array([[rows.lo[i], rhi[i], cols.lo[j], chi[j]] for i in range(rows.g) for j in range(cols.g)], dtype=np.int32)
        self._eklt_box_bound = (int((rhi - rows.lo).max()), int((chi - cols.lo).max()))

    def _eklt_needs_events(self) -> bool:
        return self._dep_thresholding

    def _eklt_canvas(self) -> Tuple[int, int]:
        return self._dep_canvas

    def _eklt_select(self, job):
        """The dependent solver's selection -> sel [b, gh, gw] int32 (0 = not selected)."""
        lib, b, dev, evs = job.lib, job.b, job.dev, job.evs
        H, W = (int(v) for v in self.orig_image_shape)
        gh, gw = self.patch_image_size
        key = "axes:" + str(dev)
        if key not in self._eklt_dev:
            self._eklt_dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in self._dep_boxes)
        rb, cb = self._eklt_dev[key]
        counts = [int(ev.shape[0]) for ev in evs] if evs else [0] * b
        sel = torch.empty(b, gh, gw, dtype=torch.int32, device=dev)
        count = torch.zeros(b, dtype=torch.int32, device=dev)
        ev_all = torch.cat(evs) if self._dep_thresholding else None
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
        check(lib.ebos_gml_dep_select_batch(b, H, W, self._dep_patch, self._dep_slide, ptr(rb), ptr(cb), ptr(ev_all), ptr(offsets),
                                            max(counts), *self._dep_canvas, int(self._dep_thresholding), self._dep_thres, ptr(sel),
                                            ptr(count), *job.tail), "ebos_gml_dep_select_batch")
        return sel

    def _eklt_flow(self, job, best_index, hyp_t) -> None:
        H, W = (int(v) for v in self.orig_image_shape)
        gh, gw = self.patch_image_size
        grid = torch.empty(job.b, 2, gh, gw, dtype=torch.float64, device=job.dev)
        check(job.lib.ebos_eklt_patch_flow_batch_f64(job.b, H, W, self._dep_patch, self._dep_slide, gh, gw, ptr(best_index), ptr(hyp_t),
                                                     int(hyp_t.shape[0]), ptr(grid), ptr(job.flow), stream_ptr(job.dev)),
              "ebos_eklt_patch_flow_batch_f64")


class GenerativeGlobalMixin(EkltSweepMixin):
    """``estimate(events, frame=..., background=...) -> np.ndarray [2, H, W]`` of the reference's GenerativeMaximumLikelihood
    (method generative_max_likelihood): one box, ``filter.parameters`` xmin .. ymax; the flow is the winner, constant over the image."""

    _gml_who = "EKLT global sweep solver"

    def _global_setup(self) -> None:
        self._eklt_setup()
        xmin, xmax, ymin, ymax = self._gml_roi
        if xmax - xmin < 1 or ymax - ymin < 1:
            raise ValueError(f"{self._gml_who}: ROI {self._gml_roi} is empty")
        self._eklt_boxes = np.array([[xmin, xmax, ymin, ymax]], dtype=np.int32)
        self._eklt_box_bound = (xmax - xmin, ymax - ymin)
        self.n_patch = 1

    def _eklt_select(self, job):
        return None

    def _eklt_flow(self, job, best_index, hyp_t) -> None:
        k = best_index[:, 0].long()
        v = hyp_t[k.clamp(min=0), :2] * (k >= 0).to(torch.float64)[:, None]   # [b, 2]; 0 where nothing won
        job.flow.copy_(v[:, :, None, None].expand_as(job.flow))


def make_patch_independent_class(base, name: str = "GenerativePatchIndependent"):
    """``GenerativePatchIndependent`` composed over ``base`` (a ``SolverBase``), with the reference's constructor signature."""
    return make_solver_class(GenerativePatchIndependentMixin, GenerativePatchIndependentMixin._patch_setup, base, name)


def make_global_class(base, name: str = "GenerativeGlobal"):
    """``GenerativeGlobal`` composed over ``base`` (a ``SolverBase``), with the reference's constructor signature."""
    return make_solver_class(GenerativeGlobalMixin, GenerativeGlobalMixin._global_setup, base, name)


GenerativePatchIndependent = make_patch_independent_class(SolverBase)
GenerativeGlobal = make_global_class(SolverBase)


def register_eklt_into(solver_module, names=("patch_eklt", "generative_max_likelihood")):
    """Add the two sampled solvers to ANOTHER solver registry -- the reference's ``src.solver`` -- built over THAT module's
    ``SolverBase``, so that ``bos_event.py`` drives ``method: patch_eklt`` and ``method: generative_max_likelihood`` unchanged.
    ``names``: (the patch solver's name, the global solver's name).  Returns the two classes."""
    patch = register_into(make_patch_independent_class(solver_module.SolverBase), solver_module, names[:1])
    glob = register_into(make_global_class(solver_module.SolverBase), solver_module, names[1:2])
    return patch, glob


__all__ = ["EkltSweepMixin", "GenerativeGlobal", "GenerativeGlobalMixin", "GenerativePatchIndependent", "GenerativePatchIndependentMixin",
           "make_global_class", "make_patch_independent_class", "parameter_keys", "register_eklt_into", "sample_table", "unfold_table"]
