"""``RecordingEvaluator.run(photometric=True)`` on the synthetic recording: the per-step photometric dicts are, bit for bit, those of
window-by-window ``photometric_error`` calls on the public interface; two more text files with one line per step; the three existing
files do not change; the frame-based flow explains frames that are at least 3 apart better than no flow does."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gml_cases as CP  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, ROI = (128, 160), (0, 128, 16, 144)


class _Viz(object):
    def __init__(self, save_dir):
        self.save_dir = str(save_dir)
        os.makedirs(self.save_dir, exist_ok=True)


def _config(stamps, dt):
    from event_based_bos_amd.utils import propagate_config

    H, W = SHAPE
    solver = copy.deepcopy(CP.solver_config("yaml_128"))
    solver["method"] = "count"
    solver["filter"] = {"filters": None, "parameters": {}}
    solver["patch_eklt"] = {"patch_size": 8, "sliding_window": 8, "do_event_thresholding": False, "event_thres": 8}
    cfg = {"common_params": {"n_frames": dt, "xmin": ROI[0], "xmax": ROI[1], "ymin": ROI[2], "ymax": ROI[3]},
           "data": {"height": H, "width": W, "remove_nose": False},
           "estimation_method": "solver", "method": "opencv_flow",
           "evaluation": {"metrics": ["flow"], "time_list": [[float(stamps[0]) + 0.004, float(stamps[-1]) + 0.004]]},
           "params_opencv_flow": {"flags": 0, "iterations": 3, "levels": 3, "poly_n": 5, "poly_sigma": 1.2, "pyr_scale": 0.5, "winsize": 10},
           "solver": solver}
    return propagate_config(cfg)


def _count_solver(cfg, save_dir):
    """A solver whose flow is a fixed function of the window's polarity counts: two runs agree bit for bit."""
    from event_based_bos_amd.solver.base import SolverBase

    class CountSolver(SolverBase):
        def estimate(self, events, *args, **kwargs):
            img = self.orig_imager.create_image_from_events_numpy(np.asarray(events), method="polarity", sigma=0)
            return np.stack([0.1 * (img[0] - img[1]), 0.025 * (img[0] + img[1])])

    d = cfg["data"]
    return CountSolver((d["height"], d["width"]), (d["crop_height"], d["crop_width"]), {}, copy.deepcopy(cfg["solver"]), _Viz(save_dir))


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    import event_based_bos_amd as ebos
    from event_based_bos_amd.evaluation import synthetic_recording

    tmp = tmp_path_factory.mktemp("photometric_eval")
    ev_path, fr_path, tr_path, stamps = synthetic_recording(str(tmp / "rec"), SHAPE, 10, 4000, seed=5)
    return ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path), stamps, tmp


def _same_dicts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in w:
            assert isinstance(g[k], np.float64)
            assert np.array_equal(np.float64(g[k]), np.float64(w[k]), equal_nan=True), (k, g[k], w[k])


@pytest.mark.parametrize("max_batch", [1, 8])
def test_evaluator_photometric(recording, max_batch):
    from event_based_bos_amd import evaluation as E, photometric as ph

    events, frames, stamps, tmp = recording
    cfg = _config(stamps, dt=3)
    off_dir, on_dir = tmp / f"off_{max_batch}", tmp / f"on_{max_batch}"
    off = E.RecordingEvaluator(cfg, events, frames, _count_solver(cfg, off_dir), save_dir=str(off_dir)).run(max_batch=max_batch)
    on = E.RecordingEvaluator(cfg, events, frames, _count_solver(cfg, on_dir), save_dir=str(on_dir)).run(
        max_batch=max_batch, photometric=True, keep_flows=True)
    assert off.photometric is None and off.photometric_reference is None
    n = len(on.steps)
    assert n >= 3 and len(on.photometric) == len(on.photometric_reference) == n

    # the flag changes nothing else: the three existing files byte for byte, and no new file without it
    for fname in (E.TEXT_WITHOUT_MASK, E.TEXT_WITH_MASK, E.TEXT_TIMESTAMPS):
        assert open(on_dir / fname, "rb").read() == open(off_dir / fname, "rb").read(), fname
    for fname in (E.TEXT_PHOTOMETRIC, E.TEXT_PHOTOMETRIC_REFERENCE):
        assert not os.path.exists(off_dir / fname)
        lines = open(on_dir / fname).read().splitlines()
        assert [ln.split("::")[0] for ln in lines] == [f"frame {i}" for i in range(n)], fname
        assert on.files[fname] == str(on_dir / fname)

    # window by window on the public interface: the un-cropped frames, the roi of common_params, the scaling of the pictures
    want, want_ref = [], []
    for s, (est, gt), period in zip(on.steps, on.flows, on.batch_time_scales):
        full, _ = frames.load_images([s.i1, s.i2], roi=None)
        pred = est.double() * torch.tensor(s.gt_time_scale / period, dtype=torch.float64, device=est.device)
        want.append(ph.photometric_error(full[0], full[1], pred, roi=ROI))
        want_ref.append(ph.photometric_error(full[0], full[1], gt, roi=ROI))
    _same_dicts(on.photometric, want)
    _same_dicts(on.photometric_reference, want_ref)
    for d in on.photometric + on.photometric_reference:
        assert list(d) == list(ph.COLUMNS) and d["n_points"] > 0

    # frames 3 apart: the frame-based flow explains the pair better than no flow
    for s, d in zip(on.steps, on.photometric_reference):
        assert s.i2 - s.i1 >= 3
        print(f"step {s.i_frame} ({s.i1} -> {s.i2}): SSIM {d['SSIM']:.4f} vs un-warped {d['SSIM_0']:.4f};  L1 {d['L1']:.3f} vs {d['L1_0']:.3f}")
        assert d["SSIM"] > d["SSIM_0"]
