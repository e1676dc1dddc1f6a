#!/usr/bin/env python
"""Run the reference driver's per-frame evaluation of a recording on the GPU (event_based_bos_amd.evaluation).

    python tools/run_eval.py --config_file tests/golden/config_hot_plate1.json --events recording.npz --frames frames/ \
        --triggers trigger_events.txt [--homography homography.txt] [--max-batch 8] [--height H --width W] [--out out/]
    python tools/run_eval.py --synthetic [--n-iter 60] [--pictures] [--photometric]
    python tools/run_eval.py --synthetic --config_file configs/cmax_time_aware_eval.yaml [--n-iter 60]
    python tools/run_eval.py --synthetic --config_file configs/eklt_patch_sweep.yaml --n-iter 64   # the sampled patch_eklt: 64 hypotheses

``--config_file`` is a JSON (or, where PyYAML is installed, YAML) file with the reference's keys; a file with an "input" section
(tests/golden/config_hot_plate1.json) is read from there and propagated.  ``--synthetic`` builds a small recording in a temporary
directory and evaluates it, so the tool runs anywhere a GPU is; with ``--config_file`` too, the synthetic recording is evaluated
with the ``solver`` section of that file (configs/cmax_time_aware_eval.yaml: the time-aware contrast maximisation as a native loop,
solved in batches through ``estimate_batch_prepared``).
"""
import argparse
import copy
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOLVERS = {"patch_eklt_pyramid2": "generative_patch_pyramid", "patch_eklt_dependent": "generative_patch_dependent",
           "patch_eklt": "generative_patch_independent", "generative_max_likelihood": "generative_global"}


def load_config(path: str) -> dict:
    with open(path) as f:
        if path.lower().endswith((".yaml", ".yml")):
            import yaml

            cfg = yaml.safe_load(f)
        else:
            cfg = json.load(f)
    return copy.deepcopy(cfg["input"]) if "input" in cfg else cfg


def synthetic_config(shape, roi, stamps, n_iter: int, solver_from: str = None) -> dict:
    """The configuration of the synthetic recording; ``solver_from``: a config file whose ``solver`` section replaces the default's."""
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = load_config(os.path.join(os.path.dirname(here), "tests", "golden", "config_hot_plate1.json"))
    if solver_from is not None:
        cfg["solver"] = copy.deepcopy(load_config(solver_from)["solver"])
        cfg["solver"].setdefault("optimizer", {})
    cfg["common_params"].update({"xmin": roi[0], "xmax": roi[1], "ymin": roi[2], "ymax": roi[3]})
    cfg["data"].update({"height": shape[0], "width": shape[1]})
    cfg["evaluation"]["time_list"] = [[float(stamps[0]) + 0.004, float(stamps[-1]) + 0.004]]
    cfg["solver"]["optimizer"]["n_iter"] = n_iter
    cfg["params_opencv_flow"]["levels"] = 3
    return cfg


def build_solver(ebos, cfg: dict):
    d = cfg["data"]
    method = cfg["solver"]["method"]
    cls = ebos.solver.collections[SOLVERS.get(method, method)]
    return cls((d["height"], d["width"]), (d["crop_height"], d["crop_width"]), {}, cfg["solver"], None)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config_file")
    ap.add_argument("--events", help=".npz of raw columns, the camera's EVT 3.0 .raw, or the reference's .hdf5 (needs h5py)")
    ap.add_argument("--frames", help="directory of image files, or a .npy / .npz stack")
    ap.add_argument("--triggers", help="trigger_events.txt (default: next to --frames; the trigger words of a .raw --events where there is none)")
    ap.add_argument("--homography", help="homography.txt: camera -> event view")
    ap.add_argument("--height", type=int)
    ap.add_argument("--width", type=int)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="directory of the three text files (default: a temporary directory)")
    ap.add_argument("--poisson", action="store_true")
    ap.add_argument("--pictures", action="store_true", help="also write the driver's ten pictures per step under --out (needs PIL)")
    ap.add_argument("--photometric", action="store_true",
                    help="also score the estimate and the frame-based flow against the frames (L1, RMSE, SSIM): two more text files")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n-iter", type=int, default=60, help="--synthetic: Adam iterations")
    args = ap.parse_args(argv)

    import event_based_bos_amd as ebos
    from event_based_bos_amd.evaluation import RecordingEvaluator, synthetic_recording

    out = args.out or tempfile.mkdtemp(prefix="ebos_eval_")
    if args.synthetic:
        shape, roi = (128, 160), (0, 128, 16, 144)
        ev_path, fr_path, tr_path, stamps = synthetic_recording(os.path.join(out, "recording"), shape, 8, 8000)
        cfg = synthetic_config(shape, roi, stamps, args.n_iter, args.config_file)
        events, frames = ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path)
    else:
        if not (args.config_file and args.events and args.frames):
            ap.error("--config_file, --events and --frames are required without --synthetic")
        cfg = load_config(args.config_file)
        if args.height:
            cfg["data"]["height"] = args.height
        if args.width:
            cfg["data"]["width"] = args.width
        triggers = args.triggers or os.path.join(os.path.dirname(os.path.abspath(args.frames.rstrip("/"))), "trigger_events.txt")
        events = ebos.RawEventStore(args.events)
        if not args.triggers and not os.path.exists(triggers) and events.triggers is not None:
            triggers = events.triggers   # the EXT_TRIGGER words of the .raw recording itself
        frames = ebos.FrameStore(args.frames, triggers, args.homography,
                                 (cfg["data"]["height"], cfg["data"]["width"]) if args.homography else None)
    cfg = ebos.utils.propagate_config(cfg)
    solv = build_solver(ebos, cfg)
    result = RecordingEvaluator(cfg, events, frames, solv, save_dir=out).run(max_batch=args.max_batch, poisson=args.poisson,
                                                                              pictures=args.pictures, photometric=args.photometric)
    print(f"{len(result.steps)} steps evaluated, {len(result.skipped)} skipped; text files in {out}")
    if args.pictures:
        print(f"  {sum(f.endswith('.png') for f in os.listdir(out))} pictures and {sum(f.endswith('.npy') for f in os.listdir(out))} flows written")
    if args.photometric:
        for name, dicts in (("estimate", result.photometric), ("frame-based", result.photometric_reference)):
            for k in ("L1", "SSIM"):
                v, v0 = np.array([d[k] for d in dicts]), np.array([d[k + "_0"] for d in dicts])
                print(f"  photometric   {name:11s} {k:4s} mean {np.nanmean(v):.6g}  (un-warped {np.nanmean(v0):.6g})")
    for name, stats in result.statistics.items():
        for k, s in stats.items():
            print(f"  {name:13s} {k:5s} mean {s['mean']:.6g}  std {s['std']:.6g}  min {s['min']:.6g}  max {s['max']:.6g}  n {s['n_data']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
