"""event_based_bos_amd -- MI355X-native contrast-maximisation inner loop for event-based BOS.

One hot path, built from scratch for gfx950 / CDNA4 behind the plugin surface of
tub-rip/event_based_bos:

    warp events (dense flow | 2-DoF)  ->  bilinear-splat image of warped events  ->  contrast cost (+ gradients)

    Warp                 drop-in for src/warp.py
    EventImageConverter  drop-in for src/event_image_converter.py
    costs                drop-in for src/costs (+ image_variance, gradient_magnitude)
    EventPlan            device-resident SoA event window + the fused warp/IWE kernels
    SlabBatch            several independent windows per launch (ebos_iwe_slab_batch_f32)
    TimeAwarePlanStack   the binned time-aware plans of several windows as one set of streams; from_raw builds them from the raw
                         sensor columns in one set of launches (ebos_plan_time_aware_raw_batch)
    solver               contrast-maximisation solver behind the reference's solver registry
    event_filters        the reference's BAF / HOT event filters and EventFilter, on the GPU
    flow_error           the reference's flow-error metrics (EPE, NPE, AE), batched, on the GPU
    poisson              the reference's Poisson integration of a flow (and its uint8 picture), batched, on fp64 matrix cores
    frame_flow           the reference's frame-based flow (cv2.calcOpticalFlowFarneback, FrameFlowEstimator), batched
    frame_warp           the reference loader's frame warp (cv2.warpPerspective) and the driver's crop, batched, one launch
    data_loader          raw-column event store (the CCS raw_events layout) feeding EventPlan.build_raw; FrameStore, the frame half
    evaluation           the reference driver's per-frame evaluation of a recording: the plan, the batched window ingest, the evaluator
    visualizer           the reference visualizer's pictures (colour-coded flow, event picture, density picture), batched
    event_voxel          the reference's event voxel grid and discretised event volume; the voxel grids of a batch of raw windows
    flow_voxel           the reference's time-aware flow: upwind / Burgers / bilinear flow voxels of one flow or a batch, and their mean
    time_bins, warp_voxel   the time-aware warp: every event displaced by the flow of its own time bin of a flow voxel
                         (Warp.warp_event(.., "dense-flow-voxel"), EventPlan.build(.., time_bin=T).iwe_voxel / contrast_voxel)
                         and its contrast maximisation as a native loop: EventPlan.variance_voxel_value_and_grad (pixel-owner
                         backward into the voxel), solver.time_aware_loop.TimeAwarePatchLoop, solver block time_aware.native
    multi-reference      one flow scored at 1 to 4 reference times from one plan: EventPlan.iwe_dense_multi / contrast_dense_multi
                         (fused="slab": the K-image slab pipeline), EventPlan.variance_multi_value_and_grad,
                         solver.multi_reference_loop.MultiReferencePatchLoop, solver block multi_reference (native: true)
    photometric          does a flow explain its two frames?  The reference's warp_image_forward / warp_image_torch and SSIM, and a
                         fused per-item score (L1, RMSE, SSIM of the warped frame against the next, and of the un-warped baseline)
    evt3                 the camera's own EVT 3.0 .raw recordings: header, GPU decode of the word stream (events and trigger edges),
                         host encoder
    recordings           every Prophesee format: EVT 2.0, EVT 2.1, EVT 3.0 .raw and .dat files, decoded on the GPU (decode_recording),
                         host encoders and file writers; RawEventStore("cd_events.raw") / RawEventStore("x_td.dat") go through it
                         (both stand on _word_stream: the .raw header, one slab decode, one file loop)
    calibration          lens calibration: CameraCalibration (K, D), its rectification map, rectified sub-pixel events from raw
                         columns, the reference's undistort_events; frame_warp.undistort_image rectifies (and warps) frames in one resample

All arithmetic of the path runs in hand-written HIP kernels reached through the C ABI of
libebos_hip.so (include/ebos_hip.h).  There is no CPU fallback: without the library or a GPU the
operators raise ``HipUnavailableError``.
"""
from ._hip import HipUnavailableError, load_library  # noqa: F401
from .warp import MotionModelKeyError, Warp  # noqa: F401
from .event_image_converter import EventImageConverter  # noqa: F401
from .event_plan import EventPlan, SlabBatch, TimeAwarePlanStack  # noqa: F401
from .data_loader import FrameStore, RawEventStore  # noqa: F401
from .frame_warp import undistort_image, undistort_image_batch, validate_image, warp_perspective, warp_perspective_batch  # noqa: F401
from .calibration import CameraCalibration, rectify_events_raw, undistort_events  # noqa: F401
from .evaluation import (EvalStep, EvaluationResult, PreparedWindows, RecordingEvaluator, plan_evaluation,  # noqa: F401
                         window_ingest_raw_batch)
from .event_voxel import create_event_voxel, event_voxel_batch, generate_discretized_event_volume  # noqa: F401
from .flow_voxel import flow_voxel_batch  # noqa: F401
from .ops import time_bins, warp_voxel  # noqa: F401
from . import calibration, costs, data_loader, evaluation, event_filters, event_voxel, evt3, flow_error, flow_voxel, frame_flow, frame_warp, fusion, ops, photometric, poisson, recordings, solver, types, utils, visualizer  # noqa: F401

__version__ = "0.1.0"
