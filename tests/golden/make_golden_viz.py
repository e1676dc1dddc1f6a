#!/usr/bin/env python3
"""Generate tests/golden/golden_viz.npz and viz_signatures.json by running the REFERENCE's ``Visualizer`` (src/visualizer.py) under
its ``SolverBase`` (src/solver/base.py:154-287) through the four picture calls of the driver (bos_event.py:202-207) on two small
synthetic steps written to a temporary directory.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_viz.py

OpenCV is absent here: ``cv2.cvtColor(COLOR_HSV2RGB)`` and ``cv2.morphologyEx(MORPH_CLOSE, cross)`` are the numpy restatements of
tests/_viz_ref.py, and the fixture carries ``shimmed = 1``.  So the fixture pins what the reference's wrapper does around them --
argument order, which flow is masked and with which mask, the shared scale of the comparison pair, the ``outer_padding`` crop, the
file names and counters, the .npy of ``save_flow`` -- and, for the two OpenCV calls, only the restatement.  The Poisson fields the
reference integrates (scipy's DSTs) are stored too, so that the centred pictures can be restated from the very same doubles.
Only arrays and names go into the fixture.
"""
import json
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference, public_surface  # noqa: E402
import _viz_ref as R  # noqa: E402

SHAPE = (30, 50)
PAD = 2
ROI = (4, 26, 6, 44)       # rows, columns of the filtered events
METHODS = ["__init__", "update_image_shape", "update_save_dir", "get_filename_from_prefix", "rollback_save_count", "reset_save_count",
           "visualize_image", "create_clipped_iwe_for_visualization", "visualize_optical_flow", "visualize_optical_flow_on_event_mask",
           "visualize_optical_flow_pred_and_gt", "color_optical_flow", "visualize_poisson_integration", "visualize_event", "save_array"]


def step_inputs(seed):
    rs = np.random.RandomState(seed)
    H, W = SHAPE
    n = 700
    ev = np.stack([rs.randint(0, H, n), rs.randint(0, W, n), np.sort(rs.uniform(0, 0.01, n)), rs.randint(0, 2, n)], axis=1).astype(np.float64)
    ev[:9, :2], ev[:9, 3] = (10, 20), 1          # a pixel that saturates both grey pictures, and one that goes to black
    ev[9:18, :2], ev[9:18, 3] = (15, 30), 0
    ev[18, :2], ev[19, :2], ev[20, :2], ev[21, :2] = (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)
    x0, x1, y0, y1 = ROI
    keep = (ev[:, 0] >= x0) & (ev[:, 0] < x1) & (ev[:, 1] >= y0) & (ev[:, 1] < y1)
    filt = ev[keep][::2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    pred = np.stack([2.5 * np.sin(yy / 7.0 + seed) + 0.3 * rs.randn(H, W), 1.5 * np.cos(xx / 9.0) + 0.3 * rs.randn(H, W)])
    gt = np.stack([2.0 * np.sin(yy / 6.0) + 0.2 * rs.randn(H, W), 3.0 * np.cos(xx / 11.0 + seed) + 0.2 * rs.randn(H, W)])
    pred[:, 12:17, 8:15] = 0.0                      # a block of exact zeros
    return ev, filt, pred, gt


def main():
    import_reference()
    cv2 = R.install_cv2_shim()
    import src.visualizer as rviz
    import src.solver.base as rbase

    rviz.cv2 = rbase.cv2 = cv2
    fields = []
    real_poisson = rviz.poisson_reconstruct

    def recording_poisson(grady, gradx, boundary):
        out = real_poisson(grady, gradx, boundary)
        fields.append(np.array(out))
        return out

    rviz.poisson_reconstruct = recording_poisson
    out = {"shimmed": np.array(1), "shape": np.array(SHAPE), "pad": np.array(PAD), "roi": np.array(ROI), "n_steps": np.array(2)}
    root = tempfile.mkdtemp()
    try:
        viz = rviz.Visualizer(SHAPE, show=False, save=True, save_dir=root)
        solv = rbase.SolverBase(SHAPE, SHAPE, {}, {"outer_padding": PAD}, viz)
        out["max_scale"] = np.array(solv.iwe_visualize_max_scale)
        for k in range(2):
            ev, filt, pred, gt = step_inputs(20250 + k)
            solv.visualize_original_sequential(ev, filt)
            solv.visualize_flows(pred, gt)
            solv.visualize_pred_sequential(filt, pred)
            solv.visualize_gt_sequential(filt, gt)
            out[f"s{k}_orig_events"], out[f"s{k}_filter_events"], out[f"s{k}_pred"], out[f"s{k}_gt"] = ev, filt, pred, gt
            out[f"s{k}_poisson_pred"], out[f"s{k}_poisson_gt"] = fields[-2], fields[-1]
            for name in R.PICTURES:
                with Image.open(os.path.join(root, f"{name}{k}.png")) as im:
                    out[f"s{k}_{name}"] = np.array(im)
            out[f"s{k}_saved_flow"] = np.load(os.path.join(root, f"pred_flow{k}.npy"))
            out[f"s{k}_files"] = np.array(sorted(os.listdir(root)))
        out["sequential_video_list"] = np.array(solv.sequential_video_list)
        out["counter_names"] = np.array(sorted(viz.prefixed_save_count))
        out["counter_values"] = np.array([viz.prefixed_save_count[n] for n in sorted(viz.prefixed_save_count)])
        # the counters on their own: default prefix, rollback, reset
        names = [viz.get_filename_from_prefix(), viz.get_filename_from_prefix(""), viz.get_filename_from_prefix("a"),
                 viz.get_filename_from_prefix("a", "npy")]
        viz.rollback_save_count("a")
        names.append(viz.get_filename_from_prefix("a"))
        viz.rollback_save_count()
        names.append(viz.get_filename_from_prefix())
        viz.reset_save_count("a")
        names.append(viz.get_filename_from_prefix("a"))
        viz.reset_save_count("all")
        names += [viz.get_filename_from_prefix(), viz.get_filename_from_prefix("original")]
        out["counter_walk"] = np.array([os.path.relpath(n, root) for n in names])
        # a flow with a NaN, a +inf and a -inf component through the colour coding alone (its Poisson picture would be all NaN)
        bad = step_inputs(7)[2]
        bad[0, 3, 4], bad[1, 5, 6], bad[0, 7, 8] = np.nan, np.inf, -np.inf
        viz._save = False
        rgb, wheel, mx = viz.color_optical_flow(bad[0], bad[1], ord=0.5)
        out["bad_flow"], out["bad_rgb"], out["bad_max"], out["wheel"] = bad, rgb, np.array(mx), wheel
        rgb1, _, mx1 = viz.color_optical_flow(bad[0], bad[1], ord=1.0)
        out["bad_rgb_ord1"], out["bad_max_ord1"] = rgb1, np.array(mx1)
        white = viz.visualize_optical_flow_on_event_mask(step_inputs(20250)[2], step_inputs(20250)[1], max_color_on_mask=False)
        out["masked_white_dense_scale"] = np.array(white)
        out["clipped_iwe_for_visualization"] = viz.create_clipped_iwe_for_visualization(step_inputs(20250)[1], max_scale=30)
        sig = public_surface(rviz.Visualizer)
        with open(os.path.join(HERE, "viz_signatures.json"), "w") as f:
            json.dump({"Visualizer": {k: sig[k] for k in METHODS}}, f, indent=1, sort_keys=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    path = os.path.join(HERE, "golden_viz.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(out)} arrays")


if __name__ == "__main__":
    warnings.filterwarnings("ignore")
    main()
