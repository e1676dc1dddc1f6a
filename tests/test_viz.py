"""CPU checks of the visualizer port (event_based_bos_amd/visualizer.py): no kernel runs here.

* tests/_viz_ref.py -- the numpy restatement the GPU tests compare the kernels with -- reproduces tests/golden/golden_viz.npz, the
  pictures the REFERENCE's ``Visualizer`` and ``SolverBase`` drew for two small steps (OpenCV's two calls shimmed by that same
  restatement: the fixture pins the wrapper, not OpenCV's bits), exactly.
* ``Visualizer`` has the reference's methods with the reference's parameters (tests/golden/viz_signatures.json), names its files and
  walks its counters as the fixture records, refuses ``show=True`` and imports without PIL.
"""
import importlib
import inspect
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _viz_ref as R  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "golden_viz.npz"))
SIG = json.load(open(os.path.join(HERE, "golden", "viz_signatures.json")))


def step(k):
    return {n: G[f"s{k}_{n}"] for n in ("orig_events", "filter_events", "pred", "gt", "poisson_pred", "poisson_gt")}


@pytest.mark.parametrize("k", [0, 1])
def test_restatement_reproduces_the_reference_pictures(k):
    s = step(k)
    got = R.step_pictures(s["orig_events"], s["filter_events"], s["pred"], s["gt"], tuple(G["shape"]), s["poisson_pred"], s["poisson_gt"],
                          pad=int(G["pad"]), max_scale=float(G["max_scale"]))
    assert sorted(got) == sorted(R.PICTURES)
    for name in R.PICTURES:
        want = G[f"s{k}_{name}"]
        assert got[name].shape == want.shape and got[name].dtype == np.uint8, name
        assert np.array_equal(got[name], want), (name, int((got[name] != want).sum()))
    H, W = (int(v) for v in G["shape"])
    assert got["original_filter"].shape == (H - 2 * int(G["pad"]), W - 2 * int(G["pad"]))    # the outer_padding crop
    assert np.array_equal(G[f"s{k}_saved_flow"], s["pred"])                                   # save_flow: [flow_x, flow_y]
    assert got["original"].min() == 0 and got["original"].max() == 255                         # both clips of the event picture are met


def test_restatement_reproduces_the_direct_calls():
    bad = G["bad_flow"]
    assert np.isnan(bad).sum() == 1 and np.isinf(bad).sum() == 2
    rgb, wheel, mx = R.color_optical_flow(bad[0], bad[1], ord=0.5)
    assert np.array_equal(rgb, G["bad_rgb"]) and np.array_equal(wheel, G["wheel"]) and mx == float(G["bad_max"])
    rgb1, _, mx1 = R.color_optical_flow(bad[0], bad[1], ord=1.0)
    assert np.array_equal(rgb1, G["bad_rgb_ord1"]) and mx1 == float(G["bad_max_ord1"])
    s = step(0)
    mask = R.integer_iwe(s["filter_events"], tuple(G["shape"])) != 0
    white = R.flow_on_event_mask(s["pred"], mask, max_color_on_mask=False, mask_color="white", mask_morph=False)
    assert np.array_equal(white, G["masked_white_dense_scale"])
    assert np.array_equal(R.clipped_iwe(R.integer_iwe(s["filter_events"], tuple(G["shape"])), 30), G["clipped_iwe_for_visualization"])


def test_hsv_restatement_basics():
    """Grey at S = 0, the six primaries at the sector starts, black at V = 0 and H = 180 wrapping to red."""
    px = np.array([[0, 0, 200], [0, 255, 255], [30, 255, 255], [60, 255, 255], [90, 255, 255], [120, 255, 255], [150, 255, 255],
                   [77, 255, 0], [180, 255, 255]], dtype=np.uint8)
    want = np.array([[200, 200, 200], [255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [0, 0, 0],
                     [255, 0, 0]], dtype=np.uint8)
    assert np.array_equal(R.hsv2rgb_u8(px), want)


def test_mask_close_restatement():
    m = np.zeros((7, 9), dtype=np.uint8)
    m[3, 2] = m[3, 4] = m[2, 3] = m[4, 3] = 1  # a one-pixel hole inside a cross closes
    m[0, 0] = m[6, 8] = 1                      # corners survive: the border never loses the erosion
    m[1, 6] = m[1, 8] = 1                      # a one-pixel gap in a row does not close under the cross
    c = R.mask_close(m)
    assert c[3, 3] == 1 and c[1, 7] == 0 and (c >= m).all()
    assert c.sum() == m.sum() + 1
    assert np.array_equal(R.mask_close(np.ones((4, 5), dtype=np.uint8)), np.ones((4, 5), dtype=np.uint8))
    assert R.mask_close(np.zeros((4, 5), dtype=np.uint8)).sum() == 0


def params_of(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def test_visualizer_surface_matches_the_reference():
    from event_based_bos_amd.visualizer import Visualizer

    for name, rec in SIG["Visualizer"].items():
        assert hasattr(Visualizer, name), name
        got, want = params_of(getattr(Visualizer, name)), rec["params"]
        assert got[:len(want)] == want, f"Visualizer.{name}: {got} != reference {want}"
        assert all(extra[2] is not None for extra in got[len(want):]), name


def test_solver_base_has_the_picture_methods():
    from event_based_bos_amd.solver.base import SolverBase

    sig = json.load(open(os.path.join(HERE, "golden", "signatures.json")))["SolverBase"]
    for name in ("create_clipped_image", "visualize_original_sequential", "visualize_flows", "visualize_pred_sequential",
                 "visualize_gt_sequential"):
        assert params_of(getattr(SolverBase, name)) == sig[name]["params"], name


def test_counters_and_file_names(tmp_path):
    from event_based_bos_amd.visualizer import Visualizer

    viz = Visualizer((30, 50), save=False, save_dir=str(tmp_path / "out"))
    assert os.path.isdir(tmp_path / "out")                              # update_save_dir creates it
    for _ in range(int(G["n_steps"])):                                  # the names one driver step asks for, in its order
        for name in R.PICTURES:
            if name == "pred_flow":
                viz.get_filename_from_prefix(name)
                viz.rollback_save_count(name)
            viz.get_filename_from_prefix(name)
    assert sorted(viz.prefixed_save_count) == list(G["counter_names"])
    assert [viz.prefixed_save_count[n] for n in sorted(viz.prefixed_save_count)] == list(G["counter_values"])
    root = viz.save_dir
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
    assert [os.path.relpath(n, root) for n in names] == list(G["counter_walk"])
    with pytest.raises(ValueError):
        viz.rollback_save_count("never_used")


def test_show_is_refused(tmp_path):
    from event_based_bos_amd.visualizer import Visualizer

    with pytest.raises(NotImplementedError):
        Visualizer((30, 50), show=True, save_dir=str(tmp_path))
    with pytest.raises(NotImplementedError):
        Visualizer((30, 50), save_dir=str(tmp_path)).visualize_event(np.zeros((3, 4)), grayscale=False)


def test_import_and_plain_use_need_no_pil(monkeypatch, tmp_path):
    kept = sys.modules.pop("event_based_bos_amd.visualizer", None)
    for name in [n for n in sys.modules if n == "PIL" or n.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)            # ``import PIL`` now raises ImportError
    try:
        fresh = importlib.import_module("event_based_bos_amd.visualizer")
        viz = fresh.Visualizer((30, 50), save=False, save_dir=str(tmp_path))
        assert viz.get_filename_from_prefix("x").endswith("x0.png")
        with pytest.raises(ImportError):
            fresh.Visualizer((30, 50), save=True, save_dir=str(tmp_path))
    finally:
        sys.modules.pop("event_based_bos_amd.visualizer", None)
        if kept is not None:
            sys.modules["event_based_bos_amd.visualizer"] = kept
            import event_based_bos_amd

            event_based_bos_amd.visualizer = kept


def test_seeds_of_the_gpu_tests_stay_inside_the_exclusion_budget():
    """The flows tests/test_gpu_viz.py draws: the share of pixels whose pre-truncation double lies within 1e-6 of an integer is far
    below the 1e-3 the GPU test allows, for the reference alone."""
    import _viz_cases as VC

    for shape in VC.SHAPES:
        for b in range(3):
            pred, gt = VC.flows(shape, b)
            for f in (pred, gt):
                ang, val, _ = R.flow_hsv_doubles(f[0], f[1], ord=0.5)
                assert 1.0 - R.comparable(ang, val).mean() <= 1e-3
