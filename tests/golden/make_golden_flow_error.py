#!/usr/bin/env python3
"""Generate tests/golden/golden_flow_error.npz by running the REFERENCE's flow-error metrics (src/utils/flow_utils.py:706-823)
on the seeded cases of tests/_flow_error_cases.py.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_flow_error.py

Stored per case: ``<case>_ref`` = the reference's values in KEYS order (float64; NaN where the reference gives NaN).  The inputs
are rebuilt from seeds by ``case_inputs``; the one input that is not, the event mask of ``solver_roi`` -- the reference's
``EventImageConverter.create_eventmask`` of ``solver_events()`` on the 720 x 1280 sensor, sliced to the ROI as
src/solver/base.py:308-309 does -- is stored bit-packed as ``solver_roi_mask_bits``.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, _stub, import_reference  # noqa: E402
from _flow_error_cases import CASES, KEYS, ROI, SENSOR_HW, case_inputs, solver_events  # noqa: E402


def reference_flow_utils():
    _stub("cv2")
    spec = importlib.util.spec_from_file_location("ref_flow_utils", f"{REF}/src/utils/flow_utils.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    fu = reference_flow_utils()
    EventImageConverter = import_reference()[1]
    out = {}
    imager = EventImageConverter(SENSOR_HW)
    mask = imager.create_eventmask(solver_events())[:, ROI["xmin"]:ROI["xmax"], ROI["ymin"]:ROI["ymax"]]
    out["solver_roi_mask_bits"] = np.packbits(np.asarray(mask, dtype=bool).ravel())
    for name, variant in CASES.items():
        gt, pred, m, ts = case_inputs(name, out)
        if variant == "numpy":
            with np.errstate(all="ignore"):
                err = fu.calculate_flow_error_numpy(gt, pred, event_mask=m)
        else:
            err = fu.calculate_flow_error_tensor(torch.from_numpy(gt), torch.from_numpy(pred), torch.from_numpy(m),
                                                 torch.from_numpy(ts))
            err = {k: float(v) for k, v in err.items()}
        out[name + "_ref"] = np.array([float(err[k]) for k in KEYS], dtype=np.float64)
        print(f"{name:14s} " + " ".join(f"{k}={v:.6g}" for k, v in zip(KEYS, out[name + "_ref"])))
    # the cases show what they are there to show
    assert np.isnan(out["pred_eq_gt_ref"][7]) and not np.isnan(out["pred_eq_gt_ref"][0])
    assert np.isnan(out["gt_special_ref"][0])
    assert np.isnan(out["pred_nan_out_ref"][0])
    assert np.isfinite(out["tensor_f32_ts_ref"]).all() and np.isfinite(out["solver_roi_ref"]).all()
    path = os.path.join(HERE, "golden_flow_error.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
