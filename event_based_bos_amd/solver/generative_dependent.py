"""The reference's single-scale generative BOS solver, ``patch_eklt_dependent`` (src/solver/patch_eklt_dependent.py on
patch_eklt.py and generative_max_likelihood.py), as a native float64 loop on the GPU (csrc/gml.hip, ``ebos_gml_dep_*``).

Per window: the model image's Sobel gradients, the blurred polarity histogram, the event-hist weights and the inverse-histogram
weights over the whole image (``ebos_gml_prepare_batch_f64``, as the pyramid); the patch selection (``ebos_gml_dep_select_batch``:
centre in the ROI and, with ``do_event_thresholding``, more than ``event_thres`` events in the patch's box, counted on a
summed-area table); the initial grid (``ebos_gml_dep_init_batch_f64``); then ``n_iter`` Adam steps (lr 0.05) of

    L = w_dn max_c sum_r |Q - P| + w_ig mean(|d_r F winv| + |d_c F winv|) + w_fn mean |T|_2   on the ROI crop,
    F = up(Sobel(x0) / 8) (Poisson model) or up(x[0:2]) (velocity model),  T = up(x[-2:]),
    P = P0 / (|P0| + 1e-4),  P0 = F0 warp(gx, T) + F1 warp(gy, T)

over the patch grid of ``patch_eklt.patch_size`` / ``sliding_window`` (``ebos_gml_dep_solve_batch_f64``).  Unselected patches hold
no parameters: their cells stay 0 and take part in the Sobel and the upsample only.  The returned flow is ``F`` over the full image.

As in the reference: the Poisson model's initial potentials come from numpy's global RandomState (one discarded draw, then one per
selected patch in row-major order); the velocity model starts at zero; the result is the parameters after the last step (the
reference's ``best_x`` aliases the leaf tensor).  Per batch the host reads back the selection counts (to draw the initial values),
then the loss histories and the flow.

``estimate_batch(windows, frames=None, background=None, max_batch=None) -> [B, 2, H, W]`` solves several windows per launch
(``ebos_gml_dep_*_batch*``), bit for bit equal to ``estimate`` on the windows in order: the selection counts of a batch are read
back once, then the initial values are drawn window by window.  Per window: ``histories``, ``params_batch``,
``estimate_indices_batch``.  ``estimate`` is a batch of one window.  The host driver is ``GenerativeMixin``'s (generative.py);
this module adds the solver's event staging and scratch size, its steps after the prepare pass, and its record fields.

Not ported: the solver's own loss-video calls (the driver's pictures: ``SolverBase.visualize_*``).  Raising ``NotImplementedError``: the angle model, ``sobel_ksize: 5``, optimizers other than
Adam, cost terms other than diff_norm / image_gradient / flow_norm_pxy.  ``model_image: black`` is a ``ValueError`` (the reference
never sets its frame).
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from .._hip import check, ptr, stream_ptr
from .._staging import to_gpu
from .base import SolverBase
from .generative import LR, GenerativeMixin, make_solver_class, register_into


class DepAxis(object):
    """One axis of prepare_patch / interpolate_dense_flow_from_patch_tensor at patch p, slide s over length L."""

    def __init__(self, L: int, p: int, s: int):
        if p < 1 or s < 1 or p > L:
            raise ValueError(f"generative dependent solver: patch {p} / slide {s} do not fit an axis of {L}")
        self.centres = np.arange(0, L - p + s, s) + p / 2
        self.g = len(self.centres)
        self.k = int(p / 2 // s) + 1
        up = (self.g + 2 * self.k) * s
        self.off = up // 2 - L // 2
        if self.off < 0 or self.off + L > up:
            raise ValueError(f"generative dependent solver: the centre crop of {L} leaves the upsampled canvas of {up} "
                             f"(patch {p}, slide {s})")
        # FlowPatch.x_min / x_max: int() truncates toward zero
        self.lo = np.array([int(c - np.ceil(p / 2)) for c in self.centres], dtype=np.int64)
        self.hi = np.array([int(c + np.floor(p / 2)) for c in self.centres], dtype=np.int64)

    def boxes(self, lo: int, hi: int) -> np.ndarray:
        """[g, 3] int32: box start, box end, centre inside [lo, hi] (both bounds inclusive)."""
        ok = ~((self.centres < lo) | (hi < self.centres))
        return np.stack([self.lo, self.hi, ok.astype(np.int64)], axis=1).astype(np.int32)


class GenerativeDependentMixin(GenerativeMixin):
    """``estimate(events, frame=..., background=...) -> np.ndarray [2, H, W]`` of the reference's PatchEkltDependent."""

    def _dep_setup(self) -> None:
        self._gml_setup(allow_velocity=True)
        mi = self._gml_cfg.get("model_image", "current")
        if mi == "black":
            raise ValueError("generative dependent solver: model_image 'black' is not handled by patch_eklt_dependent")
        pe = dict(self.slv_config.get("patch_eklt") or {})
        if "patch_size" not in pe:
            raise ValueError("generative dependent solver: patch_eklt.patch_size is required")
        self._dep_patch = int(pe["patch_size"])
        self._dep_slide = int(pe.get("sliding_window", self._dep_patch))
        self._dep_thresholding = bool(pe.get("do_event_thresholding", False))
        thr = pe.get("event_thres")
        if self._dep_thresholding and thr is None:
            raise ValueError("generative dependent solver: do_event_thresholding needs patch_eklt.event_thres")
        self._dep_thres = float(thr) if thr is not None else 0.0
        H, W = (int(v) for v in self.orig_image_shape)
        xmin, xmax, ymin, ymax = self._gml_roi
        if xmax - xmin < 3 or ymax - ymin < 3:
            raise ValueError(f"generative dependent solver: ROI {self._gml_roi} is smaller than 3 x 3")
        self._dep_rows = DepAxis(H, self._dep_patch, self._dep_slide)
        self._dep_cols = DepAxis(W, self._dep_patch, self._dep_slide)
        self.patch_image_size = (self._dep_rows.g, self._dep_cols.g)
        self.n_patch = self._dep_rows.g * self._dep_cols.g
        self.n_parameter_dim = self._gml_n_dim
        self._dep_canvas = (0, 0)   # the summed-area table of the event thresholding; without it the selection needs none
        if self._dep_thresholding:
            self._dep_canvas = (max(int(self._dep_rows.hi.max()), 0), max(int(self._dep_cols.hi.max()), 0))
        self._dep_boxes = (self._dep_rows.boxes(xmin, xmax), self._dep_cols.boxes(ymin, ymax))
        self._gml_iters = [self._gml_n_iter]   # one solve call
        self._dep_dev = {}
        self._dep_sel = None
        self._dep_x = None
        self.params_batch = []             # estimate_batch: the final parameter grid of every window of the last call
        self.estimate_indices_batch = []   # estimate_batch: the selected patches of every window of the last call

    # ------------------------------------------------------------------ results of the last window
    @property
    def estimate_indices(self) -> np.ndarray:
        """Indices (row-major over the patch grid) of the patches that got parameters in the last window."""
        if self._dep_sel is None:
            return np.zeros(0, dtype=np.int64)
        return np.nonzero(self._dep_sel.cpu().numpy().reshape(-1))[0]

    @property
    def params(self) -> np.ndarray:
        """The final parameter grid of the last window, [n_dim, gh, gw] (0 on unselected patches)."""
        return None if self._dep_x is None else self._dep_x.cpu().numpy()

    def _dep_box_tensors(self, dev):
        key = str(dev)
        if key not in self._dep_dev:
            self._dep_dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in self._dep_boxes)
        return self._dep_dev[key]

    # ------------------------------------------------------------------ the dependent solver's part of the batch driver
    _gml_who = "generative dependent solver"
    _gml_lists = {"params_batch": "params", "estimate_indices_batch": "indices"}

    def _gml_events(self, windows, prepared: bool, dev):
        """As [n, 4] lists, which the selection reads too.  The event thresholding of the selection counts events inside each
        patch's box from the event list itself; with ``do_event_thresholding`` the prepared path therefore keeps that event path
        and hands it the windows' kept events, built on the device from the raw columns (``PreparedWindows.events``) -- the same
        list ``preprocess`` yields."""
        if prepared:
            n = len(windows) if self._dep_thresholding else 0
            return [windows.events(i).to(dev).reshape(-1, 4).contiguous() for i in range(n)]
        return [to_gpu(ev, device=dev, dtype=torch.float64).reshape(-1, 4).contiguous() for ev in windows]

    def _gml_scratch_bytes(self, lib, b: int) -> Tuple[int, int]:
        geom = (*(int(v) for v in self.orig_image_shape), self._dep_patch, self._dep_slide, *self._gml_roi, *self._dep_canvas)
        stride, nbytes = int(lib.ebos_gml_dep_scratch_bytes(*geom)), int(lib.ebos_gml_dep_scratch_bytes_batch(*geom, b))
        if stride == 0 or nbytes == 0:
            raise ValueError("generative dependent solver: invalid geometry")
        return stride, nbytes

    def _gml_solve(self, job):
        """The selection (one read-back of the batch's counts), the draws in window order, the initial grid and the Adam loop ->
        (sel [b, gh, gw], x [b, n_dim, gh, gw]) on the device."""
        lib, b, dev, evs = job.lib, job.b, job.dev, job.evs
        H, W = (int(v) for v in self.orig_image_shape)
        p, s, nd = self._dep_patch, self._dep_slide, self._gml_n_dim
        gh, gw = self.patch_image_size
        counts = [int(ev.shape[0]) for ev in evs] if evs else [0] * b
        rb, cb = self._dep_box_tensors(dev)
        sel = torch.empty(b, gh, gw, dtype=torch.int32, device=dev)
        count = torch.zeros(b, dtype=torch.int32, device=dev)
        ev_all = torch.cat(evs) if self._dep_thresholding else None
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
        check(lib.ebos_gml_dep_select_batch(b, H, W, p, s, ptr(rb), ptr(cb), ptr(ev_all), ptr(offsets), max(counts), *self._dep_canvas,
                                            int(self._dep_thresholding), self._dep_thres, ptr(sel), ptr(count), *job.tail),
              "ebos_gml_dep_select_batch")
        n_sel = [int(v) for v in count.cpu().numpy()]   # read-back 1 of the batch: how many initial values each window draws
        draws = None if self._gml_velocity else np.zeros((b, gh * gw), dtype=np.float64)
        for i, ns in enumerate(n_sel):   # window by window, as successive estimate calls draw (and fail)
            if ns == 0:
                raise ValueError("generative dependent solver: no patch selected (the reference cannot start from an empty x0)")
            if draws is not None:
                np.random.random()   # len(self._initialize_velocity()): one draw, discarded
                draws[i, :ns] = np.random.random(ns) * 2. - 1
        draws_t = None if draws is None else torch.from_numpy(draws).to(dev)
        x = torch.empty(b, nd, gh, gw, dtype=torch.float64, device=dev)
        check(lib.ebos_gml_dep_init_batch_f64(b, gh, gw, nd, ptr(sel), ptr(draws_t), ptr(x), stream_ptr(dev)),
              "ebos_gml_dep_init_batch_f64")
        check(lib.ebos_gml_dep_solve_batch_f64(b, H, W, p, s, nd, *self._gml_roi, *job.model, ptr(sel), ptr(x), self._gml_n_iter, LR,
                                               ptr(job.hist), job.history_stride, ptr(job.flow), *job.tail),
              "ebos_gml_dep_solve_batch_f64")
        return sel, x

    def _gml_records(self, h: np.ndarray, solved) -> List[dict]:
        sel, x = solved
        sel_np, x_np = sel.cpu().numpy(), x.cpu().numpy()
        return [{"history": h[i], "params": x_np[i], "indices": np.nonzero(sel_np[i].reshape(-1))[0], "sel": sel[i], "x": x[i]}
                for i in range(len(h))]

    def _gml_publish_params(self, record) -> None:
        self._dep_sel, self._dep_x = record["sel"], record["x"]


def make_dependent_class(base, name: str = "GenerativePatchDependent"):
    """``GenerativePatchDependent`` composed over ``base`` (a ``SolverBase``), with the reference's constructor signature."""
    return make_solver_class(GenerativeDependentMixin, GenerativeDependentMixin._dep_setup, base, name)


GenerativePatchDependent = make_dependent_class(SolverBase)


def register_dependent_into(solver_module, names=("patch_eklt_dependent",)):
    """Add the single-scale generative solver to ANOTHER solver registry -- the reference's ``src.solver`` -- built over THAT
    module's ``SolverBase``, so that ``bos_event.py`` drives ``method: patch_eklt_dependent`` unchanged.  Returns the class."""
    return register_into(make_dependent_class(solver_module.SolverBase), solver_module, names)


__all__ = ["DepAxis", "GenerativeDependentMixin", "GenerativePatchDependent", "make_dependent_class", "register_dependent_into"]
