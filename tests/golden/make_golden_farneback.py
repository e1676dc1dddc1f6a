#!/usr/bin/env python3
"""Generate tests/golden/golden_farneback.npz by running the REFERENCE's frame-based flow, ``FrameFlowEstimator.estimate``
(src/frame_flow_estimator.py:30-95 with src/utils/frame_utils.py:117-139,160-183 and, for the two-step method, its own
``poisson_reconstruct`` on scipy, src/utils/stat_utils.py:142-199) on the seeded cases of tests/_farneback_cases.py.  Runs only
where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_farneback.py

OpenCV is absent here: ``cv2.calcOpticalFlowFarneback`` is the numpy restatement of tests/_farneback_ref.py, and the fixture
carries ``shimmed = 1``.  So the fixture pins what the reference's wrapper does around the flow -- the channel order, the
transpose, the zero padding back to the full frame, the two-step chain with its uint8 cast -- and, for the Farneback core, only the
restatement; agreement with OpenCV's own bits is not checked.

Stored per case: ``<case>_flow`` (the rows ``stored_rows(case)`` of the returned [2, H, W] flow), ``<case>_absmax``, for the
two-step cases ``<case>_p01`` / ``<case>_p02`` (the uint8 Poisson pictures the second flow is taken between), and
``<case>_frames_sum`` (an integrity check of the rebuilt inputs).  ``signatures`` holds the reference-side parameter lists.
"""
import inspect
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _stub, import_reference  # noqa: E402
import _farneback_ref as R  # noqa: E402
from _farneback_cases import CASES, case_config, case_frames, crop, stored_rows  # noqa: E402


def install_cv2_shim():
    cv2 = types.ModuleType("cv2")

    def calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
        return R.calc_optical_flow_farneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)

    cv2.calcOpticalFlowFarneback = calcOpticalFlowFarneback
    sys.modules["cv2"] = cv2
    return cv2


def main():
    import_reference()          # (installs an empty cv2 and stubs the absent packages)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        _stub("tqdm", tqdm=lambda x, *a, **k: x)
    cv2 = install_cv2_shim()
    import src.utils.frame_utils as rfu
    import src.frame_flow_estimator as rffe

    rfu.cv2 = rffe.cv2 = cv2
    calls = []
    shimmed = rfu.bos_optical_flow

    def bos_optical_flow(frame_a, frame_b, config):
        calls.append((np.array(frame_a), np.array(frame_b)))
        return shimmed(frame_a, frame_b, config)

    rfu.bos_optical_flow = bos_optical_flow
    sys.modules["src.utils"].bos_optical_flow = bos_optical_flow
    est = rffe.FrameFlowEstimator(None)
    out = {"shimmed": np.array(1)}
    for name, c in CASES.items():
        f0, f1, f2 = case_frames(name)
        cfg = case_config(name)
        calls.clear()
        flow = est.estimate(c["method"], crop(f0, c["roi"]), crop(f1, c["roi"]), crop(f2, c["roi"]), cfg)
        assert flow.dtype == np.float32 and flow.shape[0] == 2
        out[name + "_flow"] = flow[:, stored_rows(name)]
        out[name + "_absmax"] = np.abs(flow).max()
        out[name + "_frames_sum"] = np.array([float(f.astype(np.float64).sum()) for f in (f0, f1, f2)])
        if c["method"] == "opencv_flow_two_steps":
            assert len(calls) == 3 and calls[2][0].dtype == np.uint8
            out[name + "_p01"], out[name + "_p02"] = calls[2]
        print(f"{name:16s} {c['method']:22s} flow {flow.shape} max|flow| {np.abs(flow).max():.4f}", flush=True)
    sigs = {"FrameFlowEstimator.estimate": rffe.FrameFlowEstimator.estimate,
            "FrameFlowEstimator.opencv_farneback": rffe.FrameFlowEstimator.opencv_farneback,
            "FrameFlowEstimator.opencv_farneback_two_step": rffe.FrameFlowEstimator.opencv_farneback_two_step,
            "FrameFlowEstimator.__init__": rffe.FrameFlowEstimator.__init__,
            "bos_optical_flow": shimmed, "pad_to_same_resolution": rfu.pad_to_same_resolution}
    out["signatures"] = np.array(json.dumps({k: list(inspect.signature(f).parameters) for k, f in sigs.items()}))
    path = os.path.join(HERE, "golden_farneback.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    warnings.filterwarnings("ignore")
    main()
