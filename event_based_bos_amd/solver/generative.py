"""The reference's generative BOS solver, ``patch_eklt_pyramid2`` (src/solver/patch_eklt_pyramid2.py on patch_eklt_dependent.py,
patch_eklt.py and generative_max_likelihood.py), as a native float64 loop on the GPU (csrc/gml.hip).

Per window: the model image's Sobel gradients, the blurred polarity histogram Q of the events (normalised) and the inverse-histogram
weights are formed on the device (``ebos_gml_prepare_batch_f64``); then, coarse to fine over square patches of 64, 32, 16 and 8 pixels,
``n_iter // (5 - s + 1)`` Adam steps (lr 0.05) fit the per-patch Poisson potential and warp (p_x, p_y) to Q through

    L = w_dn max_c sum_r |Q M - P| + w_ig mean(|d_r(F M) winv| + |d_c(F M) winv|) + w_fn mean |T M|_2,
    F = up(Sobel(x0) / 8),  T = up(x[1:3]),  P = P0 / (|P0| + 1e-4) M,  P0 = F0 warp(gx, T) + F1 warp(gy, T)

(``ebos_gml_solve_scale_batch_f64``: seven launches per iteration, no host synchronisation inside a scale, no atomics).  The returned
flow is ``up(Sobel(x0) / 8) M`` at the finest scale.  The loss history is read once per batch.

As in the reference: the initial potentials of the coarsest scale come from numpy's global RandomState (one discarded draw, then
one per patch, laid out by a reshape, so that p_x and p_y do not start at zero); a finer scale starts from the bilinear resize of
the coarser result; a scale's result is the parameters after its last step (the reference's ``best_x`` aliases the leaf tensor);
the cached histogram is divided by its norm again at every scale when there are no event weights.

``estimate_batch(windows, frames=None, background=None, max_batch=None) -> [B, 2, H, W]`` solves several windows per launch
(``ebos_gml_*_batch_f64``: the window is the grid's z extent, so a batch issues the launches of one window).  It is defined as
equal, bit for bit, to ``estimate`` on the windows in order, the draws from numpy's global RandomState and the solver's state
afterwards included; the per-window results are in ``histories`` and ``params_per_scale_batch``.  There is one host driver:
``estimate`` is a batch of one window through the same ``*_batch*`` entries (the single-window C entries stay in the C ABI for
tools and tests; this package does not call them).  ``GenerativeMixin`` holds the driver; the dependent solver
(generative_dependent.py) overrides the event staging, the scratch size, the solve steps and the record fields.

Not ported, because they do not change the result: the per-patch ``crop_event`` loop of ``run_estimation_per_scale`` (its mask is
unused by pyramid2) and the visualisation calls (``visualize_evolution``, ``make_video``, ``visualize_scipy_history``).
Out of scope, raising ``NotImplementedError``: the angle model, the direct-velocity model (``poisson_model: false``),
``sobel_ksize: 5``, optimizers other than Adam, model images other than current / background / black, cost terms other than
diff_norm / image_gradient / flow_norm_pxy (or a weight of "inv").  ``flow_norm_pxy`` without ``optimize_warp`` is a
configuration error (``ValueError``; the reference raises KeyError).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import _hip
from .._hip import check, ptr, stream_ptr
from .._staging import to_gpu
from ..event_image_converter import EPS_NUMPY, EventImageConverter
from .base import SolverBase

PATCHES = (64, 32, 16, 8)   # prepare_pyramidal_patch(shape, 64, 8): scales 1..4, slide = patch
FINEST_SCALE = 5
TERMS = ("diff_norm", "image_gradient", "flow_norm_pxy")
MODEL_IMAGES = ("current", "background", "black")
LR = 0.05


def grid_shape(image_size, patch: int) -> Tuple[int, int]:
    """len(arange(0, L - p + p, p)) per axis."""
    return tuple(-(-int(n) // patch) for n in image_size)


def cv_gaussian_taps(sigma: float) -> torch.Tensor:
    """cv2.getGaussianKernel for cv2.GaussianBlur(ksize=None, sigmaX=sigma) on float64: size round(8 sigma + 1) | 1."""
    n = int(round(float(sigma) * 8 + 1)) | 1
    x = torch.arange(n, dtype=torch.float64) - (n - 1) * 0.5
    t = torch.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return t * (1.0 / t.sum())


def scipy_gaussian_taps(sigma: float, truncate: float = 4.0) -> torch.Tensor:
    radius = int(truncate * float(sigma) + 0.5)
    x = torch.arange(-radius, radius + 1, dtype=torch.float64)
    k = torch.exp(-0.5 / (float(sigma) ** 2) * x ** 2)
    return k / k.sum()


def _flag(cfg: dict, key: str) -> bool:
    return bool(cfg.get(key, False))


class _History(object):
    """``cost_func.get_history()`` / ``clear_history()`` of the reference's HybridCost: per Adam iteration the loss and each term."""

    def __init__(self, terms):
        self.terms = tuple(terms)
        self.clear_history()

    def clear_history(self) -> None:
        self.history = {"loss": []}
        self.history.update({k: [] for k in self.terms})

    def get_history(self) -> dict:
        return {k: list(v) for k, v in self.history.items()}


class GenerativeMixin(object):
    """``estimate(events, frame=..., background=...) -> np.ndarray [2, H, W]`` of the reference's PatchEkltPyramid2."""

    def _gml_setup(self, allow_velocity: bool = False) -> None:
        cfg = self.slv_config
        opt = cfg.get("optimizer") or {}
        gml = dict(cfg.get("generative_ml") or {})
        if opt.get("method", "Adam") != "Adam":
            raise NotImplementedError(f"generative solver: optimizer.method {opt.get('method')!r} is not supported (Adam only)")
        if _flag(gml, "angle_model"):
            raise NotImplementedError("generative solver: the angle model is not supported (poisson_model only)")
        if not _flag(gml, "poisson_model") and not allow_velocity:
            raise NotImplementedError("generative solver: the direct-velocity model (poisson_model: false) is not supported")
        if int(gml.get("sobel_ksize", 3)) != 3:
            raise NotImplementedError("generative solver: sobel_ksize 5 is not supported")
        if _flag(gml, "px-py_as-angle-magnitude"):
            raise NotImplementedError("generative solver: px-py_as-angle-magnitude needs the optuna optimizer")
        mi = gml.get("model_image", "current")
        if mi not in MODEL_IMAGES:
            raise NotImplementedError(f"generative solver: model_image {mi!r} is not supported ({', '.join(MODEL_IMAGES)})")
        cost = dict(cfg.get("cost_with_weight") or {})
        for k, w in cost.items():
            if k not in TERMS:
                raise NotImplementedError(f"generative solver: cost term {k!r} is not supported ({', '.join(TERMS)})")
            if isinstance(w, str):
                raise NotImplementedError(f"generative solver: cost weight {w!r} of {k} is not supported (numbers only)")
        self._gml_warp = _flag(gml, "optimize_warp")
        if "flow_norm_pxy" in cost and not self._gml_warp:
            raise ValueError("generative solver: flow_norm_pxy needs generative_ml.optimize_warp (it costs p_x, p_y)")
        n_iter = int(opt.get("n_iter", 0))
        if n_iter < 0:
            raise ValueError(f"generative solver: n_iter {n_iter} < 0")
        self._gml_cfg = gml
        self._gml_cost = cost
        self._gml_n_iter = n_iter
        self._gml_iters = [n_iter // (FINEST_SCALE - s + 1) for s in range(1, FINEST_SCALE)]   # Adam steps per solve call
        self._gml_velocity = not _flag(gml, "poisson_model")
        self._gml_n_dim = (4 if self._gml_warp else 2) if self._gml_velocity else (3 if self._gml_warp else 1)
        H, W = (int(v) for v in self.orig_image_shape)
        p = (cfg.get("filter") or {}).get("parameters") or {}
        if "filter" in cfg:
            roi = tuple(int(p[k]) for k in ("xmin", "xmax", "ymin", "ymax"))
        else:
            roi = (0, H, 0, W)
        xmin, xmax, ymin, ymax = roi
        roi = (max(0, min(xmin, H)), max(0, min(xmax, H)), max(0, min(ymin, W)), max(0, min(ymax, W)))
        self._gml_roi = roi
        self._gml_frame = None
        self._gml_imager = EventImageConverter((H, W), vote=str((cfg.get("iwe") or {}).get("vote", "atomic")))
        self.cost_func = _History(cost.keys())
        self.params_per_scale = {}
        self.iter_cnt = 0
        self.histories = []                # estimate_batch: cost_func.get_history() of every window of the last call
        self.params_per_scale_batch = []   # estimate_batch: params_per_scale of every window of the last call

    # ------------------------------------------------------------------ helpers
    def _gml_weights(self):
        w = [float(self._gml_cost.get(k, 0.0)) for k in TERMS]
        order = [TERMS.index(k) for k in self._gml_cost]
        return (np.array(w, dtype=np.float64), np.array(order + [0] * (3 - len(order)), dtype=np.int32), len(order))

    def _gml_set_frame(self, frame) -> None:
        self._gml_frame = to_gpu(frame, dtype=torch.float64).contiguous()

    def poisson_to_flow(self, poisson):
        """Sobel3 (replicate borders) / 8 of a [gh, gw] potential -> [2, gh, gw] (numpy in, numpy out).  The 3 x 3 stencil of the
        patch grid, outside the iteration loop."""
        t = to_gpu(poisson, dtype=torch.float64)
        k = torch.tensor([[[[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]]],
                          [[[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]]], dtype=torch.float64, device=t.device)
        x = F.pad(t.reshape(1, 1, *t.shape[-2:]), (1, 1, 1, 1), mode="replicate")
        out = (F.conv2d(x, k) / 8.)[0]
        return out.cpu().numpy() if isinstance(poisson, np.ndarray) else out

    # ------------------------------------------------------------------ estimate, estimate_batch, estimate_batch_prepared
    _gml_who = "generative solver"
    _gml_lists = {"params_per_scale_batch": "params_per_scale"}   # per-window list (beside ``histories``) -> its field of a record

    def estimate(self, events, *args, frame=None, background=None, **kwargs) -> np.ndarray:
        """One window -> [2, H, W]: a batch of one through the batch driver.  Publishes the window as the last one (``cost_func``,
        the parameters, ``iter_cnt``) and leaves the per-window lists as the last ``estimate_batch`` call left them."""
        windows, frames, _ = self._gml_batch_args([events], frame, background, None, single=True)
        return self._gml_run(windows, frames, 1, per_window=False)[0]

    def _gml_batch_args(self, windows, frames, background, max_batch, single: bool = False):
        """The argument checks of all three entry points, before any GPU work and before any state changes -> (windows, frames,
        max_batch): ``frames`` is None (the kept background), one frame for every window, or a list of one frame per window.
        ``single``: ``frames`` is ``estimate``'s one frame, never a stack of them."""
        who = self._gml_who
        windows = list(windows)
        n = len(windows)
        if max_batch is None:
            max_batch = max(n, 1)
        if int(max_batch) != max_batch or max_batch < 1:
            raise ValueError(f"{who}: max_batch {max_batch!r} < 1")
        mi = self._gml_cfg.get("model_image", "current")
        H, W = (int(v) for v in self.orig_image_shape)
        if mi == "background":
            if self._gml_frame is not None or n == 0:
                return windows, None, int(max_batch)
            if background is None:
                raise ValueError(f"{who}: model_image 'background' needs background= on the first window")
            frames = background
        elif frames is None:
            if n == 0:
                return windows, None, int(max_batch)
            raise ValueError(f"{who}: model_image {mi!r} needs frame=" + (" (for its shape)" if mi == "black" else ""))
        if single:
            frames = np.asarray(frames) if isinstance(frames, (list, tuple)) else frames
        elif not isinstance(frames, (list, tuple)) and len(np.shape(frames)) == 3:
            frames = list(frames)
        if isinstance(frames, (list, tuple)):
            if mi == "background":
                raise ValueError(f"{who}: background= is one frame")
            if len(frames) != n:
                raise ValueError(f"{who}: {len(frames)} frames for {n} windows")
            frames = list(frames)
        for f in frames if isinstance(frames, list) else [frames]:
            if tuple(np.shape(f)) != (H, W):
                raise ValueError(f"{who}: frame shape {tuple(np.shape(f))} != image shape {(H, W)}")
        return windows, frames, int(max_batch)

    def _gml_batch_frames(self, frames, lo: int, hi: int):
        """The model images of windows [lo, hi) -> (tensor [H, W] or [b, H, W], elements between windows); keeps the last one for
        the windows to come (``model_image: black`` takes the frames only for their shape)."""
        mi = self._gml_cfg.get("model_image", "current")
        H, W = (int(v) for v in self.orig_image_shape)
        if frames is None:
            return self._gml_frame, 0
        if mi == "black":
            self._gml_set_frame(np.zeros((H, W), dtype=np.float64))
            return self._gml_frame, 0
        if not isinstance(frames, list):
            self._gml_set_frame(frames)
            return self._gml_frame, 0
        stack = torch.stack([to_gpu(f, dtype=torch.float64) for f in frames[lo:hi]]).contiguous()
        self._gml_frame = stack[-1].clone()
        return stack, H * W

    def estimate_batch(self, windows, frames=None, background=None, max_batch: Optional[int] = None) -> np.ndarray:
        """``estimate`` of every window of ``windows`` (a sequence of event arrays), several windows per launch -> [B, 2, H, W].

        Equal to ``estimate(windows[i], frame=frames[i], background=background)`` for i = 0 .. B - 1 in order, bit for bit: the
        flows, the draws from numpy's global RandomState, ``iter_cnt`` and the kept background; ``cost_func`` and the parameters
        (``params_per_scale``; ``params`` / ``estimate_indices`` of the dependent solver) hold the last window's values.  Every
        window's values are in the per-window lists of the call: ``histories`` (one ``cost_func.get_history()`` dict per window)
        and ``params_per_scale_batch`` (pyramid) or ``params_batch`` and ``estimate_indices_batch`` (dependent).
        ``frames``: one per window, or one frame for all, or None where ``model_image`` allows it.
        ``max_batch`` splits the list into consecutive batches of at most that many windows (a 720 x 1280 window holds about
        100 MB on the device); the default solves all windows at once."""
        windows, frames, max_batch = self._gml_batch_args(windows, frames, background, max_batch)
        return self._gml_run(windows, frames, max_batch)

    def estimate_batch_prepared(self, prepared, frames=None, background=None, max_batch: Optional[int] = None,
                                device_out: bool = False):
        """``estimate_batch`` of windows whose event side is on the device already: ``prepared`` is an
        ``evaluation.PreparedWindows`` (``pol`` [B, 2, H, W] float64 of ``ebos_window_ingest_raw_batch``).  The upload of the events
        and the polarity splat of every window are skipped; ``pol`` goes straight into ``ebos_gml_prepare_batch_f64``.  Everything
        else is ``estimate_batch``: the flows, the per-window lists, the draws from numpy's global RandomState, ``iter_cnt``, the
        kept background and ``max_batch`` -- bit for bit what ``estimate_batch`` gives on the same windows handed over as arrays.
        ``device_out``: return the flows as a device tensor instead of a numpy array."""
        H, W = (int(v) for v in self.orig_image_shape)
        pol = prepared.pol
        if not (isinstance(pol, torch.Tensor) and pol.is_cuda and pol.dtype == torch.float64 and pol.dim() == 4
                and tuple(pol.shape[1:]) == (2, H, W)):
            raise ValueError(f"{self._gml_who}: prepared.pol must be a device float64 [B, 2, {H}, {W}] tensor")
        _, frames, max_batch = self._gml_batch_args([None] * len(prepared), frames, background, max_batch)
        return self._gml_run(prepared, frames, max_batch, out_device=pol.device if device_out else None)

    def _gml_run(self, windows, frames, max_batch: int, per_window: bool = True, out_device=None):
        """The chunk loop of all three entry points: consecutive batches of at most ``max_batch`` of ``windows`` (a list of event
        arrays, or a ``PreparedWindows``) -> the flows [B, 2, H, W], numpy or (``out_device``) a tensor there.  Publishes after
        every batch; ``per_window``: into the per-window lists as well, emptied first."""
        H, W = (int(v) for v in self.orig_image_shape)
        prepared = not isinstance(windows, list)
        if per_window:
            self.histories = []
            for name in self._gml_lists:
                setattr(self, name, [])
        flows = []
        for lo in range(0, len(windows), max_batch):
            hi = min(lo + max_batch, len(windows))
            flow, records = self._gml_solve_batch(windows.slice(lo, hi) if prepared else windows[lo:hi],
                                                  *self._gml_batch_frames(frames, lo, hi), prepared, out_device is not None)
            self._gml_publish(records, per_window)
            flows.append(flow)
        if len(flows) == 1:   # the usual case, and every ``estimate``: the batch's own array, not a copy of it
            return flows[0]
        if out_device is not None:
            return torch.cat(flows) if flows else torch.zeros((0, 2, H, W), dtype=torch.float64, device=out_device)
        return np.concatenate([np.zeros((0, 2, H, W), dtype=np.float64)] + flows)

    def _gml_history(self, h: np.ndarray) -> dict:
        """One window's history rows [iters, 4] in the shape ``cost_func.get_history()`` returns."""
        out = {"loss": list(h[:, 0])}
        out.update({k: list(h[:, 1 + TERMS.index(k)]) for k in self._gml_cost})
        return out

    def _gml_publish(self, records, per_window: bool) -> None:
        """A solved batch's records into the solver's state: the last window's in ``cost_func``, the parameters and ``iter_cnt``
        as successive ``estimate`` calls leave them; ``per_window``: every window's appended to the per-window lists."""
        if per_window:
            self.histories += [self._gml_history(r["history"]) for r in records]
            for name, field in self._gml_lists.items():
                getattr(self, name).extend(r[field] for r in records)
        self.cost_func.clear_history()
        self.cost_func.history.update(self._gml_history(records[-1]["history"]))
        self._gml_publish_params(records[-1])
        self.iter_cnt += len(records)

    def _gml_publish_params(self, record) -> None:
        self.params_per_scale = dict(record["params_per_scale"])

    # ------------------------------------------------------------------ the batch driver
    def _gml_batch_prepare(self, lib, evs, frame_t, frame_stride: int, scratch, nbytes: int, pol=None):
        """``ebos_gml_prepare_batch_f64`` of the windows ``evs`` (GPU tensors) -> (gx, gy, q, we, winv), each [b, H, W] (gx, gy
        [1, H, W] when the model image is shared).  ``pol``: the windows' polarity images [b, 2, H, W] float64 where they exist
        already (``estimate_batch_prepared``); ``evs`` is then not read."""
        gml = self._gml_cfg
        H, W = (int(v) for v in self.orig_image_shape)
        dev = frame_t.device
        if pol is None:
            pol = torch.stack([self._gml_imager._accumulate(ev, 1.0, _hip.SPLAT_POLARITY, EPS_NUMPY, torch.float64)[0]
                               for ev in evs]).contiguous()   # [b, 2, H, W]
        b = int(pol.shape[0])
        d = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=dev)
        ng = b if frame_stride else 1
        gx, gy, q, winv = d(ng, H, W), d(ng, H, W), d(b, H, W), d(b, H, W)
        use_we = _flag(gml, "weight_loss_by_event_hist")
        we = d(b, H, W) if use_we else None
        blur = cv_gaussian_taps(gml["iwe_sigma"]).to(dev) if gml.get("iwe_sigma") else None
        wtap = cv_gaussian_taps(gml["weight_sigma"]).to(dev) if use_we else None
        itap = scipy_gaussian_taps(10).to(dev) if _flag(gml, "weight_loss_by_inverse_event_hist") else None
        rad = lambda t: 0 if t is None else (t.numel() - 1) // 2
        check(lib.ebos_gml_prepare_batch_f64(b, H, W, ptr(frame_t), frame_stride, int(_flag(gml, "use_log_intensity")), ptr(pol),
                                             int(_flag(gml, "no_polarity")), ptr(blur), rad(blur), ptr(wtap), rad(wtap), ptr(itap),
                                             rad(itap), ptr(gx), ptr(gy), ptr(q), ptr(we), ptr(winv), ptr(scratch), nbytes,
                                             stream_ptr(dev)), "ebos_gml_prepare_batch_f64")
        return gx, gy, q, we, winv

    def _gml_solve_batch(self, windows, frame_t: torch.Tensor, frame_stride: int, prepared: bool = False, device_out: bool = False):
        """One batch, one launch per pass -> (flows [b, 2, H, W], one record per window).  It computes and changes nothing of the
        solver's state; ``_gml_publish`` stores.  ``prepared``: ``windows`` is a ``PreparedWindows`` (its ``pol`` replaces the
        upload and the splat).  This is the frame both solvers share: the staging, the scratch, the prepare pass, the weights /
        order / flags, the history and flow buffers, the read-back of the histories; between them ``_gml_solve``, the solver's
        own steps on a ``job`` of what they need."""
        lib = _hip.require_gpu()
        H, W = (int(v) for v in self.orig_image_shape)
        dev, gml, b = frame_t.device, self._gml_cfg, len(windows)
        pol = windows.pol.to(dev).contiguous() if prepared else None
        evs = self._gml_events(windows, prepared, dev)
        d = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=dev)
        use_we = _flag(gml, "weight_loss_by_event_hist")
        stride, nbytes = self._gml_scratch_bytes(lib, b)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _hip.on_device(dev):
            gx, gy, q, we, winv = self._gml_batch_prepare(lib, evs, frame_t, frame_stride, scratch, nbytes, pol=pol)
            weights, order, n_terms = self._gml_weights()
            w_t = torch.from_numpy(weights).to(dev)
            o_t = torch.from_numpy(order).to(dev)
            flags = ((_hip.GML_NO_POLARITY if _flag(gml, "no_polarity") else 0) | (_hip.GML_EVENT_WEIGHTS if use_we else 0) |
                     (_hip.GML_VELOCITY if self._gml_velocity else 0))   # the velocity model: the dependent solver only
            n_rows = sum(self._gml_iters)
            hist = d(b, max(n_rows, 1), 4)
            flow = d(b, 2, H, W)
            job = SimpleNamespace(
                lib=lib, b=b, dev=dev, evs=evs, use_we=use_we, q=q, hist=hist, flow=flow, scratch=scratch, nbytes=nbytes,
                # the arguments every solve entry takes: the model (flags .. winv) in front of its own, the scratch behind them
                model=(flags, ptr(w_t), ptr(o_t), n_terms, ptr(gx), ptr(gy), H * W if frame_stride else 0, ptr(q), ptr(we), ptr(winv)),
                history_stride=4 * int(hist.shape[1]), tail=(ptr(scratch), stride, nbytes, stream_ptr(dev)))
            solved = self._gml_solve(job)
        h = hist[:, :n_rows].cpu().numpy()   # the one read-back of the batch's histories
        records = self._gml_records(h, solved)
        return (flow if device_out else flow.cpu().numpy()), records

    # ------------------------------------------------------------------ what the dependent solver overrides
    def _gml_events(self, windows, prepared: bool, dev):
        """The windows' events on the device, for the polarity splat; none where ``PreparedWindows.pol`` stands in for it."""
        return None if prepared else [to_gpu(ev, device=dev, dtype=torch.float64) for ev in windows]

    def _gml_scratch_bytes(self, lib, b: int) -> Tuple[int, int]:
        """-> (bytes of one window's scratch, bytes of the batch's)."""
        H, W = (int(v) for v in self.orig_image_shape)
        return int(lib.ebos_gml_scratch_bytes(H, W, PATCHES[-1])), int(lib.ebos_gml_scratch_bytes_batch(H, W, PATCHES[-1], b))

    def _gml_solve(self, job):
        """Every scale of every window, coarse to fine: the initial values or the resize of the coarser result, the histogram's
        normalisation, ``_gml_iters[s - 1]`` Adam steps -> the parameters after each scale {s: [b, n_dim, gh, gw]} (device)."""
        lib, b = job.lib, job.b
        H, W = (int(v) for v in self.orig_image_shape)
        x, row, per_scale = None, 0, {}
        for s, (p, it) in enumerate(zip(PATCHES, self._gml_iters), start=1):
            gh, gw = grid_shape((H, W), p)
            if x is None:   # window by window, as successive estimate calls draw
                x = torch.from_numpy(np.stack([self._gml_initial(gh, gw) for _ in range(b)])).to(job.dev)
            else:
                x = F.interpolate(x, size=[gh, gw], mode="bilinear", align_corners=False).contiguous()
            if s > 1 and not job.use_we:   # the reference divides its cached histogram in place once per scale
                check(lib.ebos_gml_normalize_batch_f64(b, H * W, ptr(job.q), ptr(job.scratch), job.nbytes, stream_ptr(job.dev)),
                      "ebos_gml_normalize_batch_f64")
            check(lib.ebos_gml_solve_scale_batch_f64(b, H, W, p, self._gml_n_dim, *self._gml_roi, *job.model, ptr(x), it, LR,
                                                     ptr(job.hist[0, row:]), job.history_stride,
                                                     ptr(job.flow) if s == len(PATCHES) else None, *job.tail),
                  "ebos_gml_solve_scale_batch_f64")
            row += it
            per_scale[s] = x
        return per_scale

    def _gml_records(self, h: np.ndarray, per_scale) -> List[dict]:
        per_scale = {s: v.cpu().numpy() for s, v in per_scale.items()}
        return [{"history": h[i], "params_per_scale": {s: v[i] for s, v in per_scale.items()}} for i in range(len(h))]

    def _gml_initial(self, gh: int, gw: int) -> np.ndarray:
        """x0 of the coarsest scale from numpy's global RandomState, as run_estimation_per_scale draws it."""
        nd = self._gml_n_dim
        np.random.random()   # len(self._initialize_velocity()): one draw, discarded
        rows = []
        for _ in range(gh * gw):
            base = np.random.random() * 2. - 1
            rows.append(np.array([base, 0., 0.] if nd == 3 else [base], dtype=np.float64))
        return np.concatenate(rows).reshape((nd, gh, gw))


def make_solver_class(mixin, setup, base, name: str):
    """``mixin`` composed over ``base`` (a ``SolverBase``), with the reference's constructor signature; ``setup`` is the mixin's
    set-up method."""

    def __init__(self, orig_image_shape, crop_image_shape, calibration_parameter=None, solver_config=None, visualize_module=None):
        base.__init__(self, orig_image_shape, crop_image_shape, {} if calibration_parameter is None else calibration_parameter,
                      {} if solver_config is None else solver_config, visualize_module)
        setup(self)

    return type(name, (mixin, base), {"__init__": __init__, "__doc__": mixin.__doc__, "__module__": mixin.__module__})


def register_into(cls, solver_module, names):
    for n in names:
        solver_module.collections[n] = cls
    return cls


def make_generative_class(base, name: str = "GenerativePatchPyramid"):
    """``GenerativePatchPyramid`` composed over ``base`` (a ``SolverBase``), with the reference's constructor signature."""
    return make_solver_class(GenerativeMixin, GenerativeMixin._gml_setup, base, name)


GenerativePatchPyramid = make_generative_class(SolverBase)


def register_generative_into(solver_module, names=("patch_eklt_pyramid2",)):
    """Add the generative solver to ANOTHER solver registry -- the reference's ``src.solver`` -- built over THAT module's
    ``SolverBase``, so that ``bos_event.py`` drives ``method: patch_eklt_pyramid2`` unchanged.  Returns the class."""
    return register_into(make_generative_class(solver_module.SolverBase), solver_module, names)
