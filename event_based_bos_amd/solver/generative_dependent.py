"""The reference's single-scale generative BOS solver, ``patch_eklt_dependent`` (src/solver/patch_eklt_dependent.py on
patch_eklt.py and generative_max_likelihood.py), as a native float64 loop on the GPU (csrc/gml.hip, ``ebos_gml_dep_*``).

Per window: the model image's Sobel gradients, the blurred polarity histogram, the event-hist weights and the inverse-histogram
weights over the whole image (``ebos_gml_prepare_f64``, as the pyramid); the patch selection (``ebos_gml_dep_select``: centre in
the ROI and, with ``do_event_thresholding``, more than ``event_thres`` events in the patch's box, counted on a summed-area table);
then ``n_iter`` Adam steps (lr 0.05) of

    L = w_dn max_c sum_r |Q - P| + w_ig mean(|d_r F winv| + |d_c F winv|) + w_fn mean |T|_2   on the ROI crop,
    F = up(Sobel(x0) / 8) (Poisson model) or up(x[0:2]) (velocity model),  T = up(x[-2:]),
    P = P0 / (|P0| + 1e-4),  P0 = F0 warp(gx, T) + F1 warp(gy, T)

over the patch grid of ``patch_eklt.patch_size`` / ``sliding_window`` (``ebos_gml_dep_solve_f64``).  Unselected patches hold no
parameters: their cells stay 0 and take part in the Sobel and the upsample only.  The returned flow is ``F`` over the full image.

As in the reference: the Poisson model's initial potentials come from numpy's global RandomState (one discarded draw, then one per
selected patch in row-major order); the velocity model starts at zero; the result is the parameters after the last step (the
reference's ``best_x`` aliases the leaf tensor).  Per window the host reads back the selection count (to draw the initial values),
then the loss history and the flow.

``estimate_batch(windows, frames=None, background=None, max_batch=None) -> [B, 2, H, W]`` solves several windows per launch
(``ebos_gml_dep_*_batch*``), bit for bit equal to ``estimate`` on the windows in order: the selection counts of a batch are read
back once, then the initial values are drawn window by window.  Per window: ``histories``, ``params_batch``,
``estimate_indices_batch``.

Not ported: the visualisation calls.  Raising ``NotImplementedError``: the angle model, ``sobel_ksize: 5``, optimizers other than
Adam, cost terms other than diff_norm / image_gradient / flow_norm_pxy.  ``model_image: black`` is a ``ValueError`` (the reference
never sets its frame).
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from .. import _hip
from .._hip import check, ptr, stream_ptr
from .._staging import to_gpu
from ..event_image_converter import EPS_NUMPY
from .base import SolverBase
from .generative import LR, GenerativeMixin, _flag, cv_gaussian_taps, scipy_gaussian_taps


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
        self._dep_canvas = (max(int(self._dep_rows.hi.max()), 0), max(int(self._dep_cols.hi.max()), 0))
        self._dep_boxes = (self._dep_rows.boxes(xmin, xmax), self._dep_cols.boxes(ymin, ymax))
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

    # ------------------------------------------------------------------ estimate
    def estimate(self, events, *args, frame=None, background=None, **kwargs) -> np.ndarray:
        mi = self._gml_cfg.get("model_image", "current")
        if "frame" in kwargs and frame is None:
            frame = kwargs["frame"]
        if mi == "current":
            if frame is None:
                raise ValueError("generative dependent solver: model_image 'current' needs frame=")
            self._gml_set_frame(frame)
        elif self._gml_frame is None:
            if background is None:
                raise ValueError("generative dependent solver: model_image 'background' needs background= on the first window")
            self._gml_set_frame(background)
        lib = _hip.require_gpu()
        H, W = (int(v) for v in self.orig_image_shape)
        if tuple(self._gml_frame.shape) != (H, W):
            raise ValueError(f"generative dependent solver: frame shape {tuple(self._gml_frame.shape)} != image shape {(H, W)}")
        dev = self._gml_frame.device
        gml = self._gml_cfg
        p, s = self._dep_patch, self._dep_slide
        gh, gw = self.patch_image_size
        nd = self._gml_n_dim
        xmin, xmax, ymin, ymax = self._gml_roi
        ev = to_gpu(events, device=dev, dtype=torch.float64).reshape(-1, 4).contiguous()
        pol = self._gml_imager._accumulate(ev, 1.0, _hip.SPLAT_POLARITY, EPS_NUMPY, torch.float64)[0].contiguous()  # [2, H, W]
        d = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=dev)
        gx, gy, q, winv = d(H, W), d(H, W), d(H, W), d(H, W)
        use_we = _flag(gml, "weight_loss_by_event_hist")
        we = d(H, W) if use_we else None
        blur = cv_gaussian_taps(gml["iwe_sigma"]).to(dev) if gml.get("iwe_sigma") else None
        wtap = cv_gaussian_taps(gml["weight_sigma"]).to(dev) if use_we else None
        itap = scipy_gaussian_taps(10).to(dev) if _flag(gml, "weight_loss_by_inverse_event_hist") else None
        hc, wc = self._dep_canvas if self._dep_thresholding else (0, 0)
        nbytes = int(lib.ebos_gml_dep_scratch_bytes(H, W, p, s, xmin, xmax, ymin, ymax, hc, wc))
        if nbytes == 0:
            raise ValueError("generative dependent solver: invalid geometry")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rad = lambda t: 0 if t is None else (t.numel() - 1) // 2
        rb, cb = self._dep_box_tensors(dev)
        sel = torch.empty(gh, gw, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        with _hip.on_device(dev):
            sp = stream_ptr(dev)
            check(lib.ebos_gml_prepare_f64(H, W, ptr(self._gml_frame), int(_flag(gml, "use_log_intensity")), ptr(pol),
                                           int(_flag(gml, "no_polarity")), ptr(blur), rad(blur), ptr(wtap), rad(wtap), ptr(itap),
                                           rad(itap), ptr(gx), ptr(gy), ptr(q), ptr(we), ptr(winv), ptr(scratch), nbytes, sp),
                  "ebos_gml_prepare_f64")
            check(lib.ebos_gml_dep_select(H, W, p, s, ptr(rb), ptr(cb), ptr(ev), int(ev.shape[0]), hc, wc, int(self._dep_thresholding),
                                          self._dep_thres, ptr(sel), ptr(count), ptr(scratch), nbytes, sp), "ebos_gml_dep_select")
            n_sel = int(count.item())   # read-back 1: how many initial values to draw
            if n_sel == 0:
                raise ValueError("generative dependent solver: no patch selected (the reference cannot start from an empty x0)")
            draws = None
            if not self._gml_velocity:
                np.random.random()   # len(self._initialize_velocity()): one draw, discarded
                draws = torch.from_numpy(np.random.random(n_sel) * 2. - 1).to(dev)
            x = d(nd, gh, gw)
            check(lib.ebos_gml_dep_init_f64(gh, gw, nd, ptr(sel), ptr(draws), ptr(x), sp), "ebos_gml_dep_init_f64")
            weights, order, n_terms = self._gml_weights()
            w_t = torch.from_numpy(weights).to(dev)
            o_t = torch.from_numpy(order).to(dev)
            flags = ((_hip.GML_NO_POLARITY if _flag(gml, "no_polarity") else 0) | (_hip.GML_EVENT_WEIGHTS if use_we else 0) |
                     (_hip.GML_VELOCITY if self._gml_velocity else 0))
            it = self._gml_n_iter
            hist = d(max(it, 1), 4)
            flow = d(2, H, W)
            check(lib.ebos_gml_dep_solve_f64(H, W, p, s, nd, xmin, xmax, ymin, ymax, flags, ptr(w_t), ptr(o_t), n_terms, ptr(gx), ptr(gy),
                                             ptr(q), ptr(we), ptr(winv), ptr(sel), ptr(x), it, LR, ptr(hist), ptr(flow), ptr(scratch),
                                             nbytes, sp), "ebos_gml_dep_solve_f64")
        h = hist[:it].cpu().numpy()   # read-back 2: the history
        self.cost_func.clear_history()
        self.cost_func.history["loss"] = list(h[:, 0])
        for k in self._gml_cost:
            self.cost_func.history[k] = list(h[:, 1 + ("diff_norm", "image_gradient", "flow_norm_pxy").index(k)])
        self._dep_sel, self._dep_x = sel, x
        self.iter_cnt += 1
        return flow.cpu().numpy()


    # ------------------------------------------------------------------ estimate_batch
    _gml_who = "generative dependent solver"

    def estimate_batch(self, windows, frames=None, background=None, max_batch=None) -> np.ndarray:
        self.params_batch, self.estimate_indices_batch = [], []
        return GenerativeMixin.estimate_batch(self, windows, frames=frames, background=background, max_batch=max_batch)

    estimate_batch.__doc__ = GenerativeMixin.estimate_batch.__doc__.replace("``params_per_scale_batch``",
                                                                            "``params_batch``, ``estimate_indices_batch``")

    def _gml_prepared_reset(self) -> None:
        GenerativeMixin._gml_prepared_reset(self)
        self.params_batch, self.estimate_indices_batch = [], []

    def _gml_solve_batch(self, windows, frame_t: torch.Tensor, frame_stride: int, prepared: bool = False, device_out: bool = False):
        """One batch: selection (one read-back of the counts), the draws in window order, the Adam loop, one launch per pass.
        ``prepared``: ``windows`` is a ``PreparedWindows``; its ``pol`` replaces the upload and the splat.  The event thresholding
        of the selection counts events inside each patch's box from the event list itself (``ebos_gml_dep_select_batch``); with
        ``do_event_thresholding`` the prepared path therefore keeps that event path and hands it the windows' kept events, built
        on the device from the raw columns (``PreparedWindows.events``) -- the same list ``preprocess`` yields."""
        lib = _hip.require_gpu()
        H, W = (int(v) for v in self.orig_image_shape)
        dev, gml, b = frame_t.device, self._gml_cfg, len(windows)
        p, s = self._dep_patch, self._dep_slide
        gh, gw = self.patch_image_size
        nd, G = self._gml_n_dim, gh * gw
        xmin, xmax, ymin, ymax = self._gml_roi
        pol = windows.pol.to(dev).contiguous() if prepared else None
        if prepared:
            evs = [windows.events(i).to(dev).reshape(-1, 4).contiguous() for i in range(b)] if self._dep_thresholding else []
        else:
            evs = [to_gpu(ev, device=dev, dtype=torch.float64).reshape(-1, 4).contiguous() for ev in windows]
        counts = [int(ev.shape[0]) for ev in evs] if evs else [0] * b
        d = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=dev)
        use_we = _flag(gml, "weight_loss_by_event_hist")
        hc, wc = self._dep_canvas if self._dep_thresholding else (0, 0)
        stride = int(lib.ebos_gml_dep_scratch_bytes(H, W, p, s, xmin, xmax, ymin, ymax, hc, wc))
        nbytes = int(lib.ebos_gml_dep_scratch_bytes_batch(H, W, p, s, xmin, xmax, ymin, ymax, hc, wc, b))
        if stride == 0 or nbytes == 0:
            raise ValueError("generative dependent solver: invalid geometry")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rb, cb = self._dep_box_tensors(dev)
        sel = torch.empty(b, gh, gw, dtype=torch.int32, device=dev)
        count = torch.zeros(b, dtype=torch.int32, device=dev)
        with _hip.on_device(dev):
            sp = stream_ptr(dev)
            gx, gy, q, we, winv = self._gml_batch_prepare(lib, evs, frame_t, frame_stride, scratch, nbytes, pol=pol)
            ev_all = torch.cat(evs) if self._dep_thresholding else None
            offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
            check(lib.ebos_gml_dep_select_batch(b, H, W, p, s, ptr(rb), ptr(cb), ptr(ev_all), ptr(offsets), max(counts), hc, wc,
                                                int(self._dep_thresholding), self._dep_thres, ptr(sel), ptr(count), ptr(scratch),
                                                stride, nbytes, sp), "ebos_gml_dep_select_batch")
            n_sel = [int(v) for v in count.cpu().numpy()]   # read-back 1 of the batch: how many initial values each window draws
            draws = None if self._gml_velocity else np.zeros((b, G), dtype=np.float64)
            for i, ns in enumerate(n_sel):   # window by window, as successive estimate calls draw (and fail)
                if ns == 0:
                    raise ValueError("generative dependent solver: no patch selected (the reference cannot start from an empty x0)")
                if draws is not None:
                    np.random.random()   # len(self._initialize_velocity()): one draw, discarded
                    draws[i, :ns] = np.random.random(ns) * 2. - 1
            draws_t = None if draws is None else torch.from_numpy(draws).to(dev)
            x = d(b, nd, gh, gw)
            check(lib.ebos_gml_dep_init_batch_f64(b, gh, gw, nd, ptr(sel), ptr(draws_t), ptr(x), sp), "ebos_gml_dep_init_batch_f64")
            weights, order, n_terms = self._gml_weights()
            w_t = torch.from_numpy(weights).to(dev)
            o_t = torch.from_numpy(order).to(dev)
            flags = ((_hip.GML_NO_POLARITY if _flag(gml, "no_polarity") else 0) | (_hip.GML_EVENT_WEIGHTS if use_we else 0) |
                     (_hip.GML_VELOCITY if self._gml_velocity else 0))
            it = self._gml_n_iter
            rows = max(it, 1)
            hist = d(b, rows, 4)
            flow = d(b, 2, H, W)
            check(lib.ebos_gml_dep_solve_batch_f64(b, H, W, p, s, nd, xmin, xmax, ymin, ymax, flags, ptr(w_t), ptr(o_t), n_terms,
                                                   ptr(gx), ptr(gy), H * W if frame_stride else 0, ptr(q), ptr(we), ptr(winv),
                                                   ptr(sel), ptr(x), it, LR, ptr(hist), rows * 4, ptr(flow), ptr(scratch), stride,
                                                   nbytes, sp), "ebos_gml_dep_solve_batch_f64")
        h = hist[:, :it].cpu().numpy()   # read-back 2: the histories
        sel_np, x_np = sel.cpu().numpy(), x.cpu().numpy()
        for i in range(b):
            self.histories.append(self._gml_history(h[i]))
            self.params_batch.append(x_np[i])
            self.estimate_indices_batch.append(np.nonzero(sel_np[i].reshape(-1))[0])
        self.cost_func.clear_history()
        self.cost_func.history.update(self._gml_history(h[-1]))
        self._dep_sel, self._dep_x = sel[-1], x[-1]
        return flow if device_out else flow.cpu().numpy()


def make_dependent_class(base, name: str = "GenerativePatchDependent"):
    """``GenerativePatchDependent`` composed over ``base`` (a ``SolverBase``), with the reference's constructor signature."""

    def __init__(self, orig_image_shape, crop_image_shape, calibration_parameter=None, solver_config=None, visualize_module=None):
        base.__init__(self, orig_image_shape, crop_image_shape, {} if calibration_parameter is None else calibration_parameter,
                      {} if solver_config is None else solver_config, visualize_module)
        self._dep_setup()

    return type(name, (GenerativeDependentMixin, base),
                {"__init__": __init__, "__doc__": GenerativeDependentMixin.__doc__, "__module__": __name__})


GenerativePatchDependent = make_dependent_class(SolverBase)


def register_dependent_into(solver_module, names=("patch_eklt_dependent",)):
    """Add the single-scale generative solver to ANOTHER solver registry -- the reference's ``src.solver`` -- built over THAT
    module's ``SolverBase``, so that ``bos_event.py`` drives ``method: patch_eklt_dependent`` unchanged.  Returns the class."""
    cls = make_dependent_class(solver_module.SolverBase)
    for n in names:
        solver_module.collections[n] = cls
    return cls


__all__ = ["DepAxis", "GenerativeDependentMixin", "GenerativePatchDependent", "make_dependent_class", "register_dependent_into"]
