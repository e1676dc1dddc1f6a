"""Event-array helpers of the path (reference: src/utils/event_utils.py).

Only ``crop_event`` is on the path: it selects the events of a region of interest (the CROP filter,
src/utils/event_filters.py:182-202) and of a patch (src/solver/patch_eklt.py:118-124).  The per-patch use -- one pass
over the whole event array per patch, only to count -- is replaced by ``EventPlan.patch_event_counts``.

The reference's event filters are re-exported from ``event_filters`` under their names, as src/utils/__init__.py:2 does, and
its flow-error metrics from ``flow_error``, as src/utils/__init__.py:20-21 does, and its Poisson integration and
``standardize_image_center`` from ``poisson``, as src/utils/__init__.py:34,54 does, and ``bos_optical_flow`` and
``pad_to_same_resolution`` from ``frame_flow``, as src/utils/__init__.py:34-42 does, and the two time-resolved event representations,
``create_event_voxel`` and ``generate_discretized_event_volume``, from ``event_voxel``, as src/utils/__init__.py:4,7 does, and the
time-aware flow (``construct_dense_flow_voxel_*`` and the functions around it) from ``flow_voxel``, as src/utils/__init__.py:19-33 does,
and the frame warps ``warp_image_forward`` / ``warp_image_torch`` and ``SSIM`` / ``ssim`` from ``photometric``, as
src/utils/__init__.py:40-41,54 does, and ``undistort_events`` (src/utils/event_utils.py:242-266) from ``calibration``, with the fused
frame rectification ``undistort_image`` / ``undistort_image_batch`` of ``frame_warp`` beside it.

``propagate_config`` is the driver's config plumbing for this path (reference: src/utils/config_utils.py:42-88): the
solver reads its region of interest from keys that only exist after that propagation.
"""
from .types import NUMPY_TORCH

ROI_KEYS = ("xmin", "xmax", "ymin", "ymax")


def propagate_config(config: dict) -> dict:
    """In place, like the reference's (src/utils/config_utils.py:42-88): the region of interest of ``common_params``
    (x = rows, y = columns) is copied into ``data`` and ``solver.filter.parameters``; ``data.crop_height / crop_width``,
    the ``pad_{x0,x1,y0,y1}`` margins (into ``solver`` and every ``params_<frame method>`` section), ``solver.crop_*``,
    ``solver.params_opencv_flow / params_openpiv`` and ``evaluation.dt = common_params.n_frames`` are derived.  Missing
    optional sections (``solver.filter``, ``params_*``) are created instead of raising ``KeyError``.  Returns ``config``."""
    common, data = config["common_params"], config["data"]
    solver = config.get("solver")
    for key in ROI_KEYS:
        data[key] = common[key]
        if solver is not None:
            solver.setdefault("filter", {}).setdefault("parameters", {})[key] = common[key]
    data["crop_height"] = data["xmax"] - data["xmin"]
    data["crop_width"] = data["ymax"] - data["ymin"]
    pad = {"pad_x0": common["xmin"], "pad_x1": data["height"] - common["xmax"],
           "pad_y0": common["ymin"], "pad_y1": data["width"] - common["ymax"]}
    if solver is not None:
        for sect in ("params_opencv_flow", "params_openpiv"):
            if sect in config:
                solver[sect] = config[sect]
        solver.update(pad)
        solver["crop_height"], solver["crop_width"] = data["crop_height"], data["crop_width"]
    if "evaluation" in config and "n_frames" in common:
        config["evaluation"]["dt"] = common["n_frames"]
    for k in ("opencv_flow", "openpiv", "rife", "flowformer"):
        if f"params_{k}" in config:
            config[f"params_{k}"].update(pad)
        else:
            config[f"params_{k}"] = dict(pad)
    return config


def crop_event(events: NUMPY_TORCH, x0: int, x1: int, y0: int, y1: int) -> NUMPY_TORCH:
    """Events with ``x0 <= x < x1`` and ``y0 <= y < y1`` (x = row = events[..., 0], y = column = events[..., 1]);
    numpy arrays and torch tensors on any device, order kept.  src/utils/event_utils.py:109-129."""
    mask = (x0 <= events[..., 0]) & (events[..., 0] < x1) & (y0 <= events[..., 1]) & (events[..., 1] < y1)
    return events[mask]


def remove_event(events: NUMPY_TORCH, x0: int, x1: int, y0: int, y1: int) -> NUMPY_TORCH:
    """The complement of ``crop_event``: the events outside rows [x0, x1) x columns [y0, y1), order kept (the driver's
    ``remove_nose``).  src/utils/event_utils.py:133-153."""
    mask = (x0 <= events[..., 0]) & (events[..., 0] < x1) & (y0 <= events[..., 1]) & (events[..., 1] < y1)
    return events[~mask]


from .event_filters import (EventFilter, background_activity_filter, continuous_background_activity_filter,  # noqa: E402,F401
                            hot_pixel_filter)
from .flow_error import calculate_flow_error_numpy, calculate_flow_error_tensor, flow_error_batch  # noqa: E402,F401
from .poisson import (poisson_image, poisson_reconstruct, poisson_reconstruct_batch,  # noqa: E402,F401
                      standardize_image_center)
from .frame_flow import bos_optical_flow, pad_to_same_resolution  # noqa: E402,F401
from .event_voxel import create_event_voxel, generate_discretized_event_volume  # noqa: E402,F401
from .flow_voxel import (construct_dense_flow_voxel_numpy, construct_dense_flow_voxel_torch,  # noqa: E402,F401
                         convert_flow_per_bin_to_flow_per_sec, flow_voxel_batch, inviscid_burger_flow_to_voxel_numpy,
                         inviscid_burger_flow_to_voxel_torch, propagate_flow_to_voxel_numpy, propagate_flow_to_voxel_torch,
                         truncate_voxel_flow_numpy, upwind_flow_to_voxel_numpy, upwind_flow_to_voxel_torch)
from .photometric import SSIM, ssim, warp_image_forward, warp_image_torch  # noqa: E402,F401
from .calibration import undistort_events  # noqa: E402,F401
from .frame_warp import undistort_image, undistort_image_batch  # noqa: E402,F401
