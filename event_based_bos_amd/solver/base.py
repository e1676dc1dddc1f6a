"""``SolverBase`` -- the solver plugin surface the driver talks to (reference: src/solver/base.py:54-378).

Kept from the reference: the constructor signature, ``preprocess(events) -> (events, time_period)``,
``estimate(events, *args, **kwargs) -> np.ndarray [2, H, W]`` and the owned helpers ``orig_imager`` /
``crop_imager`` / ``orig_warper`` / ``crop_warper`` (always ``normalize_t=True``, :98-100).  The driver's picture calls
(``visualize_original_sequential`` / ``visualize_flows`` / ``visualize_pred_sequential`` / ``visualize_gt_sequential``, :208-287) are
composed over ``visualize_module`` exactly as the reference composes them: ``visualizer.Visualizer`` of this package renders on the
GPU, the reference's own ``Visualizer`` works there too.  The driver's evaluation calls ``calculate_flow_error`` / ``save_flow_error_as_text``
(:289-353) are here, on the GPU metrics of ``flow_error``.  ``preprocess`` runs the reference's
filter pipeline (src/solver/base.py:108-139): CROP to the region of interest, then the filters ``solver.filter.filters``
lists ("BAF", "HOT": ``event_filters.EventFilter`` on the GPU, the BAF time map carried from window to window when
BAF_continuous_update is set).  A config without a ``filters`` list only crops, exactly as before.
"""
from __future__ import annotations

import logging
import os
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _hip, costs, event_filters, event_image_converter, flow_error, warp
from .._staging import to_gpu

logger = logging.getLogger(__name__)


class SolverBase(object):
    """Args (same positions/names as the reference):
        orig_image_shape (tuple) ... (H, W) of the sensor.
        crop_image_shape (tuple) ... (H, W) of the region of interest.
        calibration_parameter (dict | None) ... unused by this path, stored.
        solver_config (dict) ... the ``solver`` section of the YAML.
        visualize_module ... optional object, stored as ``visualizer``.
    """

    def __init__(self, orig_image_shape: tuple, crop_image_shape: tuple, calibration_parameter: Optional[dict] = None,
                 solver_config: Optional[dict] = None, visualize_module=None):
        self.orig_image_shape = tuple(orig_image_shape)
        self.crop_image_shape = tuple(crop_image_shape)
        self.calib_param = calibration_parameter
        self.slv_config = dict(solver_config or {})
        self.visualizer = visualize_module
        self.sequential_video_list: list = []
        self.evaluation_text_list: list = []
        self.pad = int(self.slv_config.get("outer_padding", 0))
        self.vote = str((self.slv_config.get("iwe") or {}).get("vote", "atomic"))   # iwe: {vote: ordered}: bit-identical repeats
        self.orig_imager = event_image_converter.EventImageConverter(self.orig_image_shape, outer_padding=self.pad, vote=self.vote)
        self.crop_imager = event_image_converter.EventImageConverter(self.crop_image_shape, outer_padding=self.pad, vote=self.vote)
        self.orig_warper = warp.Warp(self.orig_image_shape, normalize_t=True, calib_param=calibration_parameter)
        self.crop_warper = warp.Warp(self.crop_image_shape, normalize_t=True, calib_param=calibration_parameter)
        self.warp_direction = self.slv_config.get("warp_direction", "first")
        self.motion_model = self.slv_config.get("motion_model", "dense-flow")
        self.roi = self._roi_from_config(self.slv_config)
        self.filter_set = self._filter_from_config(self.orig_image_shape, self.slv_config)
        self.previous_best = None
        self.iwe_visualize_max_scale = self.slv_config.get("max_scale", 50)
        self._viz_imager = event_image_converter.EventImageConverter(self.orig_image_shape, vote=self.vote)   # (the reference's orig_imager: no padding)

    @staticmethod
    def _filter_from_config(image_shape, cfg: dict) -> Optional[event_filters.EventFilter]:
        """The reference's ``setup_filter_preprocess`` (src/solver/base.py:108-121): an ``EventFilter`` of the ``solver.filter``
        section when it lists filters (an unknown name raises KeyError here); None when it lists none -- CROP alone."""
        section = cfg.get("filter") or {}
        if not section.get("filters"):
            return None
        return event_filters.EventFilter(image_shape, section)

    @staticmethod
    def _roi_from_config(cfg: dict) -> Optional[Tuple[int, int, int, int]]:
        """(xmin, xmax, ymin, ymax) of the CROP filter; x = rows, y = columns
        (keys propagated by src/utils/config_utils.py:42-88 into solver.filter.parameters)."""
        p = (cfg.get("filter") or {}).get("parameters") or {}
        keys = ("xmin", "xmax", "ymin", "ymax")
        return tuple(int(p[k]) for k in keys) if all(k in p for k in keys) else None

    def preprocess(self, events) -> tuple:
        """CROP the window to the ROI, then the listed BAF / HOT filters, and report its time period -- that of the cropped
        window (src/solver/base.py:123-139)."""
        ev = to_gpu(events)
        if self.filter_set is not None and ev.shape[0] < event_filters.MIN_EVENTS:
            return events, float((ev[:, 2].max() - ev[:, 2].min()).item()) if ev.shape[0] else 0.0  # (EventFilter.process: as it is)
        if self.roi is not None:
            x0, x1, y0, y1 = self.roi
            keep = (ev[:, 0] >= x0) & (ev[:, 0] < x1) & (ev[:, 1] >= y0) & (ev[:, 1] < y1)
            ev = ev[keep]
        period = float((ev[:, 2].max() - ev[:, 2].min()).item()) if ev.shape[0] else 0.0
        if self.filter_set is not None:
            ev = self.filter_set.process(ev, skip=("CROP",) if self.roi is not None else ())
        if isinstance(events, np.ndarray):
            return ev.cpu().numpy(), period
        return (ev if events.is_cuda else ev.cpu()), period

    def estimate(self, events, *args, **kwargs) -> np.ndarray:
        raise NotImplementedError

    # ------------------------------------------------------------------ pictures (src/solver/base.py:154-287)
    def create_clipped_image(self, events, max_scale=50):
        """255 - uint8(clip(max_scale IWE, 0, 255)) of the un-padded bilinear vote of ``events`` [n, 4], ``outer_padding`` pixels
        cropped from every side -> uint8 numpy [H - 2 pad, W - 2 pad] (:154-174; rendered by csrc/visualize.hip)."""
        from ..visualizer import clipped_iwe_picture

        assert events.shape[-1] <= 4, "this function is for events"
        ev = to_gpu(events, dtype=torch.float64)
        iwe = self._viz_imager._accumulate(ev, 1.0, _hip.SPLAT_BILINEAR, event_image_converter.EPS_NUMPY, torch.float64)
        return clipped_iwe_picture(iwe.reshape(1, *self.orig_image_shape), max_scale, self.pad)[0].cpu().numpy()

    def _listed(self, prefix: str) -> None:
        if prefix not in self.sequential_video_list:
            self.sequential_video_list.append(prefix)

    def visualize_original_sequential(self, orig_events, filter_events):
        """The event picture of ``orig_events`` ("original") and the clipped IWE of ``filter_events`` ("original_filter"), :208-227."""
        self.visualizer.visualize_event(orig_events, file_prefix="original")
        self._listed("original")
        clipped_iwe = self.create_clipped_image(filter_events, max_scale=self.iwe_visualize_max_scale)
        self.visualizer.visualize_image(clipped_iwe, file_prefix="original_filter")
        self._listed("original_filter")

    def visualize_pred_sequential(self, events, flow):
        """"pred_flow" (+ its .npy), "pred_flow_poisson" and "pred_masked" of the prediction ``flow`` [2, H, W], :229-250."""
        self.visualizer.visualize_optical_flow(flow[0], flow[1], visualize_color_wheel=False, file_prefix="pred_flow", save_flow=True)
        self._listed("pred_flow")
        self.visualizer.visualize_poisson_integration(flow, file_prefix="pred_flow_poisson")
        self._listed("pred_flow_poisson")
        self.visualizer.visualize_optical_flow_on_event_mask(flow, events, file_prefix="pred_masked", mask_color="black", mask_morph=True)
        self._listed("pred_masked")

    def visualize_gt_sequential(self, events, gt_flow):
        """"gt_flow", "gt_flow_poisson" and "gt_masked" of the reference flow ``gt_flow`` [2, H, W], :252-273."""
        self.visualizer.visualize_optical_flow(gt_flow[0], gt_flow[1], visualize_color_wheel=False, file_prefix="gt_flow", save_flow=False)
        self._listed("gt_flow")
        self.visualizer.visualize_poisson_integration(gt_flow, file_prefix="gt_flow_poisson")
        self._listed("gt_flow_poisson")
        self.visualizer.visualize_optical_flow_on_event_mask(gt_flow, events, file_prefix="gt_masked", mask_color="black", mask_morph=True)
        self._listed("gt_masked")

    def visualize_flows(self, pred_flow, gt_flow) -> None:
        """"flow_comparison_pred" and "flow_comparison_gt" on one scale (+ the colour wheel), :276-287."""
        self.visualizer.visualize_optical_flow_pred_and_gt(pred_flow, gt_flow, pred_file_prefix="flow_comparison_pred",
                                                           gt_file_prefix="flow_comparison_gt")

    def calculate_flow_error(self, pred_disp, gt_flow, timescale: float = 1.0, events=None, roi: Optional[dict] = None) -> dict:
        """Flow error of one window (src/solver/base.py:289-318): ``flow_error.calculate_flow_error_numpy(gt_flow[None],
        pred_disp[None], event_mask)`` on the GPU.

        Args:
            pred_disp, gt_flow ... [2, H, W] pixel displacements (numpy or torch; an ROI view is read in place on the device).
            timescale ... only logged, as in the reference.
            events ... optional [n, 4] events: the mask is ``orig_imager.create_eventmask`` of them as a float64 device tensor,
                sliced ``[:, xmin:xmax, ymin:ymax]`` with ``roi``; it never leaves the device.  (The reference hands numpy
                events to create_eventmask, whose bilinear weights drop contributions below 1e-8 instead of 1e-6: the masks
                differ only for events within 1e-6 of a pixel boundary.)
            roi ... dict with xmin, xmax, ymin, ymax (rows, columns), required with ``events`` as in the reference.
        Returns:
            {"EPE", "1PE", "2PE", "3PE", "5PE", "10PE", "20PE", "AE"}: np.float64 values.
        """
        event_mask = None
        if events is not None:
            ev = to_gpu(events, dtype=torch.float64)
            event_mask = self.orig_imager.create_eventmask(ev)[:, roi["xmin"]:roi["xmax"], roi["ymin"]:roi["ymax"]]
        err = flow_error.calculate_flow_error_numpy(gt_flow[None], pred_disp[None], event_mask=event_mask)
        logger.info(f"{err = } for time period {timescale} sec.")
        return err

    def save_flow_error_as_text(self, nth_frame: int, flow_error_dict: dict, fname: str = "flow_error_per_frame.txt"):
        """Append ``frame <n>::{...}`` to ``fname`` (under ``visualizer.save_dir`` when there is a visualizer) and list the file in
        ``evaluation_text_list`` (src/solver/base.py:340-353).  Numeric values are written as plain Python floats: under numpy >= 2
        the reference's own writer emits ``np.float64(...)``, which its reader ``read_flow_error_text`` (src/utils/misc.py:88-113:
        "nan" -> "0.0", then ``ast.literal_eval``) cannot parse; these lines it can."""
        if self.visualizer is not None:
            save_file_name = os.path.join(self.visualizer.save_dir, fname)
        else:
            save_file_name = fname
        plain = {k: _plain(v) for k, v in flow_error_dict.items()}
        with open(save_file_name, "a") as f:
            f.write(f"frame {nth_frame}::" + str(plain) + "\n")
        if save_file_name not in self.evaluation_text_list and fname != "timestamps_per_frame.txt":
            self.evaluation_text_list.append(save_file_name)

    def set_previous_frame_best_estimation(self, previous_best):
        self.previous_best = previous_best  # warm start hook (src/solver/base.py:355-361)


def _plain(v):
    """A numpy / torch scalar as a plain Python number (so that ``str`` of it is a literal); anything else unchanged."""
    if isinstance(v, torch.Tensor) and v.numel() == 1:
        v = v.item()
    if isinstance(v, np.generic):
        v = v.item()
    return v
