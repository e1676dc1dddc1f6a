"""The visualizer's pictures on the GPU (event_based_bos_amd/visualizer.py, csrc/visualize.hip) against the numpy restatement of
tests/_viz_ref.py (which tests/test_viz.py pins to the reference's own pictures).

1. 8-bit HSV -> RGB: all 181 x 256 (H, V) pairs at S = 255 (and a sweep of S), bit for bit.
2. The cross-shaped mask close: exact on random masks of density 0.02 / 0.3 / 0.9, on corners and edges, alone and batched.
3. Event picture, clipped IWE and the padding crop (0 and 2): exact on integer-pixel events.
4. Flow colour, masked colour, shared-scale pair, centred picture: equal to the restatement on the same doubles, all channels,
   except where the restatement's pre-truncation double (the angle, 255 mag / max, a / max|a| 127 + 128) lies within 1e-6 of an
   integer -- device atan2 / sqrt may differ from libm in the last bit there.  The left-out share is asserted <= 1e-3 per image.
   A pixel with value 0 is black whatever its hue and is compared.
5. ``render_step_batch`` at B = 3 equals its B = 1 calls bit for bit; ``RecordingEvaluator.run(pictures=True)`` writes the
   reference's file set, the decoded files are the rendered arrays, and the error dicts are those of ``pictures=False``.
6. ``SolverBase``'s picture methods over this package's ``Visualizer`` draw the pictures of the fixture's steps (rule of 4).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _viz_cases as VC  # noqa: E402
import _viz_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(HERE, "golden", "golden_viz.npz"))
BUDGET = 1e-3


@pytest.fixture(scope="module")
def V():
    from event_based_bos_amd import visualizer
    return visualizer


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def assert_equal_where(got, want, ok, what):
    left_out = 1.0 - ok.mean()
    bad = (got != want)
    if bad.ndim == 3:
        bad = bad.any(axis=2)
    print(f"{what}: left out {left_out:.2e} of {ok.size} pixels, {int((bad & ok).sum())} differ among the compared, "
          f"{int((bad & ~ok).sum())} among the left out")
    assert left_out <= BUDGET, (what, left_out)
    assert not (bad & ok).any(), (what, int((bad & ok).sum()))


# ------------------------------------------------------------------------------------------------ 1
def test_hsv_to_rgb_exhaustive(V):
    h, v = np.meshgrid(np.arange(181), np.arange(256), indexing="ij")
    hsv = np.stack([h, np.full_like(h, 255), v], axis=-1).astype(np.uint8)
    assert np.array_equal(V.hsv_to_rgb(hsv), R.hsv2rgb_u8(hsv))
    got = V.hsv_to_rgb(dev(hsv))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), R.hsv2rgb_u8(hsv))
    rs = np.random.RandomState(4)
    anyb = rs.randint(0, 256, (4001, 3)).astype(np.uint8)       # every byte is accepted: hue above 180, any saturation; odd count
    anyb[:256, 1] = 0
    assert np.array_equal(V.hsv_to_rgb(anyb), R.hsv2rgb_u8(anyb))


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("shape", VC.SHAPES + [(17, 131)])
def test_mask_close(V, shape):
    masks = VC.masks(shape)
    want = np.stack([R.mask_close(m) for m in masks])
    got = V.mask_close(masks)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    for k in (0, 3):
        assert np.array_equal(V.mask_close(dev(masks[k])).cpu().numpy(), want[k])                  # B = 1, [H, W]
    assert np.array_equal(V.mask_close(masks.astype(bool)), want)
    assert (want[3] >= masks[3]).all() and want[4].sum() == 0 and want[5].all()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("shape", VC.SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_event_picture_and_clipped_iwe(V, shape, B):
    ev = [VC.events(shape, b) for b in range(B)]
    oc = np.stack([VC.counts(e[0], shape) for e in ev])
    fc = np.stack([VC.counts(e[1], shape) for e in ev])
    got = V.event_picture(dev(oc)).cpu().numpy()
    want = np.stack([R.event_picture(*R.signed_counts(e[0], shape)) for e in ev])
    assert np.array_equal(got, want) and want.min() == 0 and want.max() == 255
    assert np.array_equal(V.event_picture(dev(oc), 100).cpu().numpy(), np.stack([R.event_picture(c[0], c[1], 100) for c in oc]))
    for pad in (0, 2, 3):
        for scale in (50, 7.5):
            got = V.clipped_iwe_picture(dev(fc[:, 0]), scale, pad, second=dev(fc[:, 1])).cpu().numpy()
            want = np.stack([R.clipped_iwe(R.integer_iwe(e[1], shape), scale, pad) for e in ev])
            assert got.shape == (B, shape[0] - 2 * pad, shape[1] - 2 * pad) and np.array_equal(got, want), (pad, scale)
    one = V.clipped_iwe_picture(dev(fc.sum(1)), 50, 2).cpu().numpy()                                  # one plane, no second
    assert np.array_equal(one, np.stack([R.clipped_iwe(R.integer_iwe(e[1], shape), 50, 2) for e in ev]))


def test_visualize_event_and_clipped_iwe_methods(V, tmp_path):
    shape = VC.SHAPES[0]
    viz = V.Visualizer(shape, save_dir=str(tmp_path))
    ev, filt = VC.events(shape, 0)
    out = ev.copy()
    out[5, 0], out[6, 1], out[7, 0] = -3.0, shape[1] + 8.0, shape[0] - 0.4          # clipped into the image, then truncated
    for e in (ev, out):
        got = viz.visualize_event(e)
        assert isinstance(got, np.ndarray) and np.array_equal(got, R.event_picture(*R.signed_counts(e, shape)))
    signed = ev.copy()
    signed[:, 3] = signed[:, 3] * 2 - 1
    assert np.array_equal(viz.visualize_event(signed), R.event_picture(*R.signed_counts(signed, shape)))
    assert np.array_equal(viz.visualize_event(dev(ev)).cpu().numpy(), R.event_picture(*R.signed_counts(ev, shape)))
    assert np.array_equal(viz.visualize_event(ev, ignore_polarity=True, background_color=90),
                          R.event_picture(VC.counts(ev, shape).sum(0), 0, 90))
    assert np.array_equal(viz.create_clipped_iwe_for_visualization(filt, max_scale=30), R.clipped_iwe(R.integer_iwe(filt, shape), 30))


# ------------------------------------------------------------------------------------------------ 4
def _check_color(V, flow, got, what, max_magnitude=None, ord=0.5, mask=None, multiply=False, paint=None):
    """got [H, W, 3] against the restatement of color_optical_flow on (flow * mask if multiply) with the pixels off the mask painted."""
    used = flow * mask[None] if (mask is not None and multiply) else flow
    ang, val, _ = R.flow_hsv_doubles(used[0], used[1], max_magnitude, ord)
    want = R.color_optical_flow(used[0], used[1], max_magnitude, ord)[0].copy()
    ok = R.comparable(ang, val)
    if mask is not None and paint is not None:
        want[~mask.astype(bool)] = paint
        ok = ok | ~mask.astype(bool)
    assert_equal_where(got, want, ok, what)


@pytest.mark.parametrize("shape", VC.SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_flow_pictures(V, shape, B):
    pairs = [VC.flows(shape, b) for b in range(B)]
    pred = np.stack([VC.bad_flow(shape) if b == 0 else p[0] for b, p in enumerate(pairs)])     # window 0: NaN, +inf, zeros
    gt = np.stack([p[1] for p in pairs])
    masks = np.stack([R.integer_iwe(VC.events(shape, b)[1], shape) != 0 for b in range(B)]).astype(np.uint8)
    closed = np.stack([R.mask_close(m) for m in masks])
    dp, dg, dm = dev(pred), dev(gt), dev(closed)
    for ord in (0.5, 1.0, 0.8):
        s = V.reduce_scales([V._flow_field(dp, pair=dg), V._flow_field(dp), V._flow_field(dg), V._flow_field(dp, mask=dm)], ord)
        sc = s.cpu().numpy()
        own = V.flow_rgb(dp, s[:, 1], ord=ord).cpu().numpy()
        shared_p, shared_g = V.flow_rgb(dp, s[:, 0], ord=ord).cpu().numpy(), V.flow_rgb(dg, s[:, 0], ord=ord).cpu().numpy()
        black = V.flow_rgb(dp, s[:, 3], dm, 1 | 2, ord).cpu().numpy()
        white = V.flow_rgb(dp, s[:, 1], dm, 4, ord).cpu().numpy()
        for b in range(B):
            m_p, m_g = R.magnitude(pred[b, 0], pred[b, 1], ord).max(), R.magnitude(gt[b, 0], gt[b, 1], ord).max()
            m_m = R.magnitude(pred[b, 0] * closed[b], pred[b, 1] * closed[b], ord).max()
            tol = 4e-16      # (a last bit of sqrt / pow, twice)
            for got_s, want_s in zip(sc[b], (max(m_p, m_g), m_p, m_g, m_m)):
                assert abs(got_s - want_s) <= tol * want_s, (ord, b, got_s, want_s)
            if ord == 0.8:
                continue      # (pow's last bit moves every value: the pictures are compared at the reference's two exponents)
            _check_color(V, pred[b], own[b], f"own scale {shape} b{b} ord{ord}", None, ord)
            _check_color(V, pred[b], shared_p[b], f"pair pred {shape} b{b} ord{ord}", max(m_p, m_g), ord)
            _check_color(V, gt[b], shared_g[b], f"pair gt {shape} b{b} ord{ord}", max(m_p, m_g), ord)
            _check_color(V, pred[b], black[b], f"masked black {shape} b{b} ord{ord}", None, ord, closed[b], True, 0)
            _check_color(V, pred[b], white[b], f"masked white {shape} b{b} ord{ord}", None, ord, closed[b], False, 255)
    zero = torch.zeros((1, 2) + shape, dtype=torch.float64, device="cuda")
    assert int(V.flow_rgb(zero, V.reduce_scales([V._flow_field(zero)])[:, 0]).max()) == 0           # an all-zero flow is black


@pytest.mark.parametrize("shape", VC.SHAPES)
def test_centred_picture_of_the_poisson_field(V, shape):
    from event_based_bos_amd.poisson import poisson_reconstruct_batch

    flows = np.stack([VC.flows(shape, b)[1] for b in range(3)] + [np.zeros((2,) + shape)])
    p = poisson_reconstruct_batch(dev(flows))
    s = V.reduce_scales([V._scalar_field(p)])
    got = V.centered_picture(p, s[:, 0]).cpu().numpy()
    field = p.cpu().numpy()
    for b in range(3):
        assert s[b, 0].item() == np.abs(field[b]).max()
        d = R.centered_double(field[b])
        assert_equal_where(got[b], R.trunc_u8(d), R.centered_comparable(field[b]), f"centred {shape} b{b}")
        assert got[b].min() >= 1 and (got[b].max() == 255 or got[b].min() == 1)
    assert (got[3] == 128).all()                                                                # an all-zero field
    one = V.centered_picture(p[1:2], V.reduce_scales([V._scalar_field(p[1:2])])[:, 0]).cpu().numpy()
    assert np.array_equal(one[0], got[1])


def test_visualizer_methods_against_the_restatement(V, tmp_path):
    shape = VC.SHAPES[0]
    viz = V.Visualizer(shape, save_dir=str(tmp_path))
    pred, gt = VC.flows(shape, 1)
    ev, filt = VC.events(shape, 1)
    rgb, wheel, mx = viz.color_optical_flow(pred[0], pred[1])
    assert mx == R.magnitude(pred[0], pred[1], 1.0).max() and np.array_equal(wheel, R.color_wheel(shape[0])) and wheel.shape == (30, 30, 3)
    _check_color(V, pred, rgb, "color_optical_flow", None, 1.0)
    rgb2, _, mx2 = viz.color_optical_flow(dev(pred[0]), dev(pred[1]), max_magnitude=2.0 * mx, ord=1.0)
    assert mx2 == 2.0 * mx and rgb2.is_cuda
    _check_color(V, pred, rgb2.cpu().numpy(), "color_optical_flow(max)", 2.0 * mx, 1.0)
    a, b = viz.visualize_optical_flow_pred_and_gt(pred, gt)
    m = max(R.magnitude(pred[0], pred[1], 0.5).max(), R.magnitude(gt[0], gt[1], 0.5).max())
    _check_color(V, pred, a, "pred_and_gt pred", m, 0.5)
    _check_color(V, gt, b, "pred_and_gt gt", m, 0.5)
    mask = R.integer_iwe(filt, shape) != 0
    got = viz.visualize_optical_flow_on_event_mask(pred, filt, mask_color="black", mask_morph=True)
    _check_color(V, pred, got, "on_event_mask", None, 0.5, R.mask_close(mask), True, 0)
    got = viz.visualize_optical_flow_on_event_mask(pred, filt, max_color_on_mask=False)
    _check_color(V, pred, got, "on_event_mask dense", None, 0.5, mask.astype(np.uint8), False, 255)
    assert os.listdir(tmp_path) == []                                                           # save=False writes nothing


# ------------------------------------------------------------------------------------------------ 5
def _step_inputs(shape, B):
    pred = np.stack([VC.flows(shape, b)[0] for b in range(B)])
    gt = np.stack([VC.flows(shape, b)[1] for b in range(B)])
    ev = [VC.events(shape, b) for b in range(B)]
    oc = np.stack([VC.counts(e[0], shape) for e in ev])
    fc = np.stack([VC.counts(e[1], shape) for e in ev])
    return pred, gt, (fc.sum(1) != 0).astype(np.uint8), fc, oc, ev


@pytest.mark.parametrize("shape", VC.SHAPES)
def test_render_step_batch(V, shape):
    from event_based_bos_amd.poisson import poisson_reconstruct_batch

    pred, gt, mask, fc, oc, ev = _step_inputs(shape, 3)
    pred[0] = VC.bad_flow(shape)
    batch = V.render_step_batch(dev(pred), dev(gt), dev(mask), dev(fc), dev(oc), outer_padding=2, max_scale=50, return_poisson=True)
    assert sorted(k for k in batch if not k.startswith("poisson_")) == sorted(V.PICTURES)
    for b in range(3):
        one = V.render_step_batch(pred[b], gt[b], mask[b], fc[b], oc[b], outer_padding=2, max_scale=50)
        for name in V.PICTURES:
            assert one[name].dtype == torch.uint8 and np.array_equal(one[name][0].cpu().numpy(), batch[name][b].cpu().numpy()), (name, b)
    for b in (1, 2):      # against the restatement, on the Poisson fields the device integrated
        want = R.step_pictures(ev[b][0], ev[b][1], pred[b], gt[b], shape, batch["poisson_pred"][b].cpu().numpy(),
                               batch["poisson_gt"][b].cpu().numpy(), pad=2, max_scale=50)
        for name in ("original", "original_filter"):
            assert np.array_equal(batch[name][b].cpu().numpy(), want[name]), name
        for name in V.PICTURES[2:]:
            differ = (batch[name][b].cpu().numpy() != want[name])
            differ = differ.any(axis=-1) if differ.ndim == 3 else differ
            assert differ.mean() <= BUDGET, (name, b, differ.mean())       # (pixel by pixel with the exclusion rule: tests 4 and 6)
    assert np.array_equal(batch["poisson_gt"].cpu().numpy(), poisson_reconstruct_batch(dev(gt)).cpu().numpy())


def test_evaluator_writes_the_reference_file_set(V, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import run_eval

    import event_based_bos_amd as ebos
    from event_based_bos_amd.evaluation import RecordingEvaluator, synthetic_recording

    shape, roi = (128, 160), (0, 128, 16, 144)
    ev_path, fr_path, tr_path, stamps = synthetic_recording(str(tmp_path / "rec"), shape, 7, 4000)
    cfg = ebos.utils.propagate_config(run_eval.synthetic_config(shape, roi, stamps, 6))
    events, frames = ebos.RawEventStore(ev_path), ebos.FrameStore(fr_path, tr_path)
    results = {}
    for pictures in (False, True):
        np.random.seed(3)
        out = tmp_path / f"out_{int(pictures)}"
        solv = run_eval.build_solver(ebos, cfg)
        results[pictures] = RecordingEvaluator(cfg, events, frames, solv, save_dir=str(out)).run(max_batch=3, pictures=pictures)
        if pictures:
            assert solv.sequential_video_list == [n for n in V.PICTURES if not n.startswith("flow_comparison")]
    plain, drawn = results[False], results[True]
    n = len(drawn.steps)
    assert n >= 3 and plain.pictures is None and len(drawn.pictures) == n
    assert plain.timestamps == drawn.timestamps
    for key in ("errors_without_mask", "errors_with_mask"):
        for a, b in zip(getattr(plain, key), getattr(drawn, key)):
            assert list(a) == list(b) and all(np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True) for k in a), key
    texts = sorted(os.listdir(tmp_path / "out_0"))
    for t in texts:
        assert open(tmp_path / "out_0" / t).read() == open(tmp_path / "out_1" / t).read(), t
    want_files = sorted(texts + [f"{name}{k}.png" for name in V.PICTURES for k in range(n)] + [f"pred_flow{k}.npy" for k in range(n)]
                        + ["color_wheel.png"])
    assert sorted(os.listdir(tmp_path / "out_1")) == want_files
    per_step = [f for f in G["s0_files"] if f != "color_wheel.png"]
    assert sorted(per_step) == sorted([f"{name}0.png" for name in V.PICTURES] + ["pred_flow0.npy"])   # the reference's own set
    for k in range(n):
        for name in V.PICTURES:
            with Image.open(tmp_path / "out_1" / f"{name}{k}.png") as im:
                assert np.array_equal(np.array(im), drawn.pictures[k][name]), (name, k)
        saved = np.load(tmp_path / "out_1" / f"pred_flow{k}.npy")
        assert saved.shape == (2,) + shape and saved.dtype == np.float64
    with Image.open(tmp_path / "out_1" / "color_wheel.png") as im:
        assert np.array_equal(np.array(im), R.color_wheel(shape[0]))


# ------------------------------------------------------------------------------------------------ 6
class _Recorder(object):
    """A ``Visualizer`` that keeps what it would write (no PIL): {file name: picture}."""

    @staticmethod
    def make(V, shape, save_dir):
        class Recording(V.Visualizer):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self._save, self.written = True, {}

            def _show_or_save_image(self, image, file_prefix=None, fixed_file_name=None):
                name = f"{fixed_file_name}.png" if fixed_file_name is not None else self.get_filename_from_prefix(file_prefix)
                self.written[os.path.basename(name)] = np.array(image)

        return Recording(shape, save=False, save_dir=save_dir)


def test_solver_base_draws_the_fixture_steps(V, tmp_path):
    from event_based_bos_amd.solver.base import SolverBase

    shape, pad = tuple(int(v) for v in G["shape"]), int(G["pad"])
    viz = _Recorder.make(V, shape, str(tmp_path))
    solv = SolverBase(shape, shape, {}, {"outer_padding": pad}, viz)
    for k in range(int(G["n_steps"])):
        ev, filt, pred, gt = (G[f"s{k}_{n}"] for n in ("orig_events", "filter_events", "pred", "gt"))
        solv.visualize_original_sequential(ev, filt)
        solv.visualize_flows(pred, gt)
        solv.visualize_pred_sequential(filt, pred)
        solv.visualize_gt_sequential(filt, gt)
        assert sorted(list(viz.written) + [f"pred_flow{j}.npy" for j in range(k + 1)]) == sorted(G[f"s{k}_files"])
        assert np.array_equal(np.load(tmp_path / f"pred_flow{k}.npy"), G[f"s{k}_saved_flow"])
        mask = R.mask_close(R.integer_iwe(filt, shape) != 0)
        m = max(R.magnitude(pred[0], pred[1], 0.5).max(), R.magnitude(gt[0], gt[1], 0.5).max())
        for name in ("original", "original_filter"):
            assert np.array_equal(viz.written[f"{name}{k}.png"], G[f"s{k}_{name}"]), name
        for name, flow, mx, msk in (("flow_comparison_pred", pred, m, None), ("flow_comparison_gt", gt, m, None), ("pred_flow", pred, None, None),
                                    ("gt_flow", gt, None, None), ("pred_masked", pred, None, mask), ("gt_masked", gt, None, mask)):
            used = flow if msk is None else flow * msk[None]
            ang, val, _ = R.flow_hsv_doubles(used[0], used[1], mx, 0.5)
            ok = R.comparable(ang, val) if msk is None else (R.comparable(ang, val) | (msk == 0))
            assert_equal_where(viz.written[f"{name}{k}.png"], G[f"s{k}_{name}"], ok, f"step {k} {name}")
        for name, which in (("pred_flow_poisson", "poisson_pred"), ("gt_flow_poisson", "poisson_gt")):
            # the device integrates with matrix products, the reference with FFTs: 1e-14 of max |P|, far inside the margin
            assert_equal_where(viz.written[f"{name}{k}.png"], G[f"s{k}_{name}"], R.centered_comparable(G[f"s{k}_{which}"]), f"step {k} {name}")
    assert np.array_equal(viz.written["color_wheel.png"], G["wheel"])
    assert solv.sequential_video_list == list(G["sequential_video_list"])
    assert sorted(viz.prefixed_save_count) == list(G["counter_names"])
    assert [viz.prefixed_save_count[n] for n in sorted(viz.prefixed_save_count)] == list(G["counter_values"])
    assert solv.create_clipped_image(dev(G["s0_filter_events"])).shape == (shape[0] - 2 * pad, shape[1] - 2 * pad)
