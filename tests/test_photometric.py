"""The photometric check of a flow (event_based_bos_amd/photometric.py, csrc/photometric.hip): frame warp, SSIM, the fused score.

CPU: the restatement tests/_photometric_ref.py is pinned to the reference's own outputs (golden_photometric.npz) exactly, in float64
and in float32; the host-made window taps equal the reference's ``create_window``; signatures, re-exports, refusals, no CPU
fallback.  GPU: the kernels against the restatement.

The tolerance is measured per case against the reference, never taken from the kernel: r = the largest absolute difference between
the restatement run in float32 and run in float64 on the same inputs.  A float32 kernel result must lie within 4 r of the float64
restatement, a float64 kernel result within 4 r 2^-29 (a reordered sum of the same addends differs from the reference by a small
multiple of its own rounding noise; README 4.20's rule).  Every comparison prints its ratio to the bar before it asserts.
"""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _photometric_cases as PC  # noqa: E402
import _photometric_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = (("f64", torch.float64), ("f32", torch.float32))
F64_FACTOR = 2.0 ** -29


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_photometric.npz"), allow_pickle=False))


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None or t.dtype == torch.uint8 else t.to(dtype)


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


# ================================================================================================ CPU
def test_restatement_warp_equals_the_reference(golden):
    for name in PC.GOLDEN_WARP:
        im, flow = PC.warp_inputs(name)
        for tag, dt in DTYPES:
            if tag == "f32" and name in PC.GOLDEN_WARP_F64_ONLY:
                continue
            got = R.warp_forward(_t(im), _t(flow, dt))
            assert got.dtype == dt and _same(got.double().numpy(), golden[f"{name}_{tag}"]), (name, tag)
        if name in PC.GOLDEN_WARP_NUMPY:
            assert _same(R.warp_forward(_t(im), _t(flow)).numpy(), golden[name + "_np"]), name
    assert np.isnan(golden["w_23x19_nonfinite_f64"]).sum() == 2       # (the reference's own answer at a NaN / inf flow)


def test_restatement_shift_equals_the_reference(golden):
    for name in PC.SHIFT_CASES:
        im, shift = PC.shift_inputs(name)
        for tag, dt in DTYPES:
            got = R.warp_shift(_t(im), _t(shift, dt))
            assert got.dtype == torch.float64 and _same(got.numpy(), golden[f"{name}_{tag}"]), (name, tag)


def test_restatement_ssim_equals_the_reference(golden):
    """Where the golden file was written this difference is exactly 0, in both types.  It cannot be asserted as 0 everywhere: the
    reference's own numbers are torch's CPU ``conv2d`` and ``mean``, whose order of summation changes with the CPU (vector width,
    threads), so the same reference gives other last bits on another machine.  The bound is the per-pixel bar of the GPU tests: with
    r = the largest per-pixel difference between the float32 and the float64 map, a mean of values that each lie within 4 r (4 r 2^-29
    for float64) lies within it too."""
    for name, (B, C, _, _, ws) in PC.SSIM_CASES.items():
        a, b = PC.ssim_inputs(name)
        maps = {tag: R.ssim_map(_t(a, dt), _t(b, dt), ws).double() for tag, dt in DTYPES}
        r = float((maps["f32"] - maps["f64"]).abs().max())
        assert 0 < r < 1e-3
        for tag, dt in DTYPES:
            x, y = _t(a, dt), _t(b, dt)
            got = np.concatenate([R.ssim_reference_mean(x, y, ws, True).double().reshape(1).numpy(),
                                  R.ssim_reference_mean(x, y, ws, False).double().numpy()])
            err = np.abs(got - golden[f"{name}_{tag}"]).max()
            bar = 4 * r * (F64_FACTOR if tag == "f64" else 1.0)
            print(f"ssim restatement {tag}: {name}: |restatement - reference| {err:.3e}, bar {bar:.3e}")
            assert err <= bar, (name, tag, err, bar)


def test_window_taps_equal_create_window(golden):
    from event_based_bos_amd import photometric as ph

    for ws in (5, 11, 13):
        want = golden[f"window_{ws}"]
        for make in (ph.window_taps, R.taps):
            assert _same(make(ws, torch.float32).double().numpy(), want), ws
            t64 = make(ws, torch.float64)
            assert t64.dtype == torch.float64 and _same(t64.numpy(), want), ws   # float32-rounded products, cast last
    assert tuple(ph.window_taps().shape) == (11, 11)


def test_signatures_are_the_reference_s():
    from event_based_bos_amd import photometric as ph

    want = json.load(open(os.path.join(GOLDEN, "photometric_signatures.json")))
    mine = {"warp_image_forward": ph.warp_image_forward, "warp_image_torch": ph.warp_image_torch, "ssim": ph.ssim,
            "SSIM": ph.SSIM.__init__, "SSIM.forward": ph.SSIM.forward}
    assert sorted(want) == sorted(mine)
    for name, fn in mine.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(fn).parameters.values()]
        assert got == want[name], name


def test_exports():
    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip, build, photometric as ph, utils

    for name in ("warp_image_forward", "warp_image_torch", "SSIM", "ssim"):
        assert getattr(utils, name) is getattr(ph, name), name
    assert ebos.photometric is ph
    assert ph.COLUMNS == ("L1", "RMSE", "SSIM", "L1_0", "RMSE_0", "SSIM_0", "n_points")
    assert "photometric.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["photometric.hip"]
    assert _hip.ABI_VERSION == 2
    for entry in ("ebos_warp_image_forward_f32", "ebos_warp_image_forward_f64", "ebos_ssim_map_f32", "ebos_ssim_map_f64",
                  "ebos_photometric_batch", "ebos_photometric_scratch_bytes"):
        assert entry in _hip.SIGNATURES, entry
    sig = inspect.signature(ebos.RecordingEvaluator.run)
    assert sig.parameters["photometric"].default is False


def test_python_refusals():
    from event_based_bos_amd import photometric as ph

    im, fl = torch.zeros(6, 8, dtype=torch.float64), torch.zeros(2, 6, 8, dtype=torch.float64)
    a = torch.zeros(1, 1, 6, 8)
    cases = [
        (lambda: ph.warp_image_forward(im, fl.clone().requires_grad_()), "forward_flow requires grad: the photometric functions are forward only"),
        (lambda: ph.warp_image_forward(im.clone().requires_grad_(), fl), "im1 requires grad"),
        (lambda: ph.warp_image_forward(im, fl[:, :5]), "im1 must be [H, W] and forward_flow [2, H, W], got shapes (6, 8) and (2, 5, 8)"),
        (lambda: ph.warp_image_forward(im[None], fl), "im1 must be [H, W] and forward_flow [2, H, W]"),
        (lambda: ph.warp_image_forward(im.float(), fl), "images must be uint8 or share the flows' dtype torch.float64, got torch.float32"),
        (lambda: ph.warp_image_forward(im, fl.long()), "flows must be float32 or float64, got torch.int64"),
        (lambda: ph.warp_image_forward(im.numpy(), fl), "im1 is a numpy array but forward_flow is not"),
        (lambda: ph.warp_image_forward([[0.0]], fl), "im1 must be a numpy array or a torch tensor, got list"),
        (lambda: ph.warp_image_forward(im[:1], fl[:, :1]), "flows must be at least 2 x 2 (the base grid divides by (size - 1) / 2), got 1 x 8"),
        (lambda: ph.warp_image_forward_batch(im[None].expand(2, 6, 8), fl[None].expand(3, 2, 6, 8)), "images must be [B, H, W] or [H, W], got shape (2, 6, 8)"),
        (lambda: ph.warp_image_forward_batch(im, fl), "flows must be [B, 2, H, W] with B > 0, got shape (2, 6, 8)"),
        (lambda: ph.warp_image_torch(im, torch.zeros(3)), "im1 must be [H, W] and global_shift [2], got shapes (6, 8) and (3,)"),
        (lambda: ph.warp_image_torch(im.numpy(), torch.zeros(2)), "im1 must be a torch tensor, got ndarray"),
        (lambda: ph.warp_image_torch(im, torch.zeros(2, dtype=torch.int32)), "global_shift must be float32 or float64, got torch.int32"),
        (lambda: ph.ssim(a, a.double()), "img1 and img2 must share a dtype, got torch.float32 and torch.float64"),
        (lambda: ph.ssim(a, a[..., :7]), "img1 and img2 must both be [B, C, H, W], got shapes (1, 1, 6, 8) and (1, 1, 6, 7)"),
        (lambda: ph.ssim(a[0], a[0]), "img1 and img2 must both be [B, C, H, W]"),
        (lambda: ph.ssim(a.to(torch.uint8), a.to(torch.uint8)), "img1 and img2 must be float32 or float64, got torch.uint8"),
        (lambda: ph.ssim(a, a, window_size=10), "window_size must be a positive odd integer, got 10"),
        (lambda: ph.SSIM(window_size=4), "window_size must be a positive odd integer, got 4"),
        (lambda: ph.ssim_map(a.clone().requires_grad_(), a), "img1 requires grad"),
        (lambda: ph.ssim(a[..., :1], a[..., :1]), "img1 must be at least 2 x 2"),
        (lambda: ph.photometric_error_batch(im, im[None], fl[None], roi=(0, 4, 1.5, 3)), "roi must be four integers (xmin, xmax, ymin, ymax), got (0, 4, 1.5, 3)"),
        (lambda: ph.photometric_error_batch(im, im[None].float(), fl[None]), "frame1 and frame2 must share a dtype, got torch.float64 and torch.float32"),
        (lambda: ph.photometric_error_batch(im, im, fl[None]), "frame2 must be [B, H, W] = (1, 6, 8), got shape (6, 8)"),
        (lambda: ph.photometric_error_batch(im, im[None], fl[None], mask=torch.ones(6, 7)), "mask must be [B, H, W] = (1, 6, 8) or [H, W], got shape (6, 7)"),
        (lambda: ph.photometric_error_batch(im, im[None], fl[None], window_size=2), "window_size must be a positive odd integer, got 2"),
        (lambda: ph.photometric_error(im, im, fl[None]), "frame1 and frame2 must be [H, W] and flow [2, H, W]"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert text in str(e.value), (text, str(e.value))


def test_c_abi_refuses_before_any_launch():
    """Bad arguments come back as an error code with a message and no HIP call: usable without a GPU."""
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    lib = _hip.load_library()
    p = 0x1000   # (never read)
    I = _hip
    cases = [
        (lambda: lib.ebos_warp_image_forward_f32(p, I.IMAGE_F32, 0, p, None, 0, 1, 1, 8, p, None), -1,
         b"ebos_warp_image_forward_f32: bad shape B = 1, H = 1, W = 8 (1 <= B <= 65535, H, W >= 2, H W < 2^31)"),
        (lambda: lib.ebos_warp_image_forward_f64(p, I.IMAGE_F64, 0, p, None, 0, 1, 8, 1, p, None), -1,
         b"ebos_warp_image_forward_f64: bad shape B = 1, H = 8, W = 1 (1 <= B <= 65535, H, W >= 2, H W < 2^31)"),
        (lambda: lib.ebos_warp_image_forward_f32(None, I.IMAGE_F32, 0, p, None, 0, 1, 8, 8, p, None), -1, b"ebos_warp_image_forward_f32: NULL buffer"),
        (lambda: lib.ebos_warp_image_forward_f32(p, I.IMAGE_F32, 0, p, p, 1, 1, 8, 8, p, None), -1,
         b"ebos_warp_image_forward_f32: exactly one of flows / shifts must be given"),
        (lambda: lib.ebos_warp_image_forward_f32(p, I.IMAGE_F64, 0, p, None, 0, 1, 8, 8, p, None), -1,
         b"ebos_warp_image_forward_f32: image dtype code 2 is not built (0 = uint8, 1 = the compute type)"),
        (lambda: lib.ebos_warp_image_forward_f32(p, I.IMAGE_U8, 0, None, p, I.IMAGE_F64, 1, 8, 8, p, None), -1,
         b"ebos_warp_image_forward_f32: shift dtype code 2 is not built (1 = float32, 1 = the compute type)"),
        (lambda: lib.ebos_ssim_map_f32(p, p, p, 11, 1, 1, 8, 1, p, None, None), -1, b"ebos_ssim_map_f32: bad shape H = 8, W = 1 (both >= 2, H W < 2^31)"),
        (lambda: lib.ebos_ssim_map_f64(p, p, p, 10, 1, 1, 8, 8, p, None, None), -1, b"ebos_ssim_map_f64: window_size 10 is not a positive odd number"),
        (lambda: lib.ebos_ssim_map_f32(p, None, p, 11, 1, 1, 8, 8, p, None, None), -1, b"ebos_ssim_map_f32: NULL buffer"),
        (lambda: lib.ebos_ssim_map_f32(p, p, p, 11, 0, 1, 8, 8, p, None, None), -1, b"ebos_ssim_map_f32: bad batch B = 0, C = 1 (1 <= B C <= 65535)"),
        (lambda: lib.ebos_ssim_map_f32(p, p, p, 15, 1, 1, 8, 8, p, None, None), -3, b"ebos_ssim_map_f32: window_size 15 > 13 is not built"),
        (lambda: lib.ebos_photometric_batch(3, 0, 1, 8, 8, p, 0, p, p, p, 11, 0, 0, 0, 0, 0, None, 0, p, p, 1 << 20, None), -1,
         b"ebos_photometric_batch: dtype code 3 is not built (1 = float32, 2 = float64)"),
        (lambda: lib.ebos_photometric_batch(1, 2, 1, 8, 8, p, 0, p, p, p, 11, 0, 0, 0, 0, 0, None, 0, p, p, 1 << 20, None), -1,
         b"ebos_photometric_batch: frame dtype code 2 is not built (0 = uint8, 1 = the flow's type)"),
        (lambda: lib.ebos_photometric_batch(1, 0, 1, 1, 8, p, 0, p, p, p, 11, 0, 0, 0, 0, 0, None, 0, p, p, 1 << 20, None), -1,
         b"ebos_photometric_batch: bad shape B = 1, H = 1, W = 8 (1 <= B <= 65535, H, W >= 2, H W < 2^31)"),
        (lambda: lib.ebos_photometric_batch(1, 0, 1, 8, 8, p, 0, p, p, p, 8, 0, 0, 0, 0, 0, None, 0, p, p, 1 << 20, None), -1,
         b"ebos_photometric_batch: window_size 8 is not a positive odd number"),
        (lambda: lib.ebos_photometric_batch(1, 0, 1, 8, 8, p, 0, p, None, p, 11, 0, 0, 0, 0, 0, None, 0, p, p, 1 << 20, None), -1,
         b"ebos_photometric_batch: NULL buffer"),
        (lambda: lib.ebos_photometric_batch(1, 0, 1, 8, 8, p, 0, p, p, p, 11, 1, 5, 2, 0, 8, None, 0, p, p, 1 << 20, None), -1,
         b"ebos_photometric_batch: roi rows [5, 2) columns [0, 8) is out of order"),
        (lambda: lib.ebos_photometric_batch(1, 0, 1, 8, 8, p, 0, p, p, p, 11, 0, 0, 0, 0, 0, None, 0, p, p, 8, None), -4,
         b"ebos_photometric_batch: scratch too small (8 < 104)"),
    ]
    for call, rc, text in cases:
        assert call() == rc, text
        assert lib.ebos_last_error() == text
    assert lib.ebos_photometric_scratch_bytes(I.IMAGE_F32, 3, 37, 70) == 3 * 3 * 2 * 104      # 16 x 64 tiles
    assert lib.ebos_photometric_scratch_bytes(I.IMAGE_F64, 3, 37, 70) == 3 * 3 * 3 * 104      # 16 x 32 tiles
    assert lib.ebos_photometric_scratch_bytes(0, 3, 37, 70) == 0 and lib.ebos_photometric_scratch_bytes(I.IMAGE_F32, 3, 1, 70) == 0
    assert lib.ebos_photometric_max_window() == 13


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    from event_based_bos_amd import HipUnavailableError, photometric as ph

    im, fl = np.zeros((6, 8)), np.zeros((2, 6, 8))
    a = torch.zeros(1, 1, 6, 8)
    for call in (lambda: ph.warp_image_forward(im, fl), lambda: ph.warp_image_forward(torch.from_numpy(im), torch.from_numpy(fl)),
                 lambda: ph.warp_image_torch(torch.from_numpy(im), torch.zeros(2)), lambda: ph.warp_image_forward_batch(im, fl[None]),
                 lambda: ph.ssim(a, a), lambda: ph.ssim_map(a, a), lambda: ph.SSIM()(a, a), lambda: ph.SSIM().forward(a, a),
                 lambda: ph.photometric_error_batch(im, im[None], fl[None]), lambda: ph.photometric_error(im, im, fl)):
        with pytest.raises(HipUnavailableError):
            call()


def test_chosen_flows_stay_clear_of_tap_boundaries():
    """The n_points comparison may leave out pixels whose sample position lies within W 2^-22 of an integer (float32 and float64 may
    floor differently there): at most 1e-3 of the pixels, on every scored item that counts anything."""
    for name, ((H, W), kinds, *_rest) in PC.SCORE_CASES.items():
        flows = PC.score_inputs(name)["flow"]
        for b, kind in enumerate(kinds):
            if kind == "far":
                continue
            near = int(R.near_boundary(_t(flows[b]), W * 2.0 ** -22).sum())
            assert near <= 1e-3 * H * W, (name, b, near)


# ================================================================================================ GPU
RATIOS = {}


def _bar(what, got, want64, want32, factor=1.0):
    """got within 4 r of want64, r = max |want32 - want64| over the finite entries; NaN where and only where the restatement's is."""
    got, want64, want32 = (np.asarray(v, dtype=np.float64) for v in (got, want64, want32))
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    nan = np.isnan(want64)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    assert np.array_equal(np.isnan(want32), nan), (what, "NaN pattern of the float32 restatement")
    if nan.all():
        return
    ok = ~nan
    r = np.abs(want32[ok] - want64[ok]).max()
    err = np.abs(got[ok] - want64[ok]).max()
    ratio = err / (4 * r * factor) if r > 0 else (0.0 if err == 0 else np.inf)
    key = what.split(":")[0]
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{what}: err {err:.3e}  r {r:.3e}  err / bar {ratio:.3f}  (worst {key}: {RATIOS[key]:.3f})")
    assert ratio <= 1.0, (what, err, r, ratio)


def _cuda(a, dtype=None):
    return _t(a, dtype).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PC.WARP_CASES))
def test_warp_image_forward(name):
    from event_based_bos_amd import photometric as ph

    im, flow = PC.warp_inputs(name)
    want = {tag: R.warp_forward(_t(im), _t(flow, dt)).double().numpy() for tag, dt in DTYPES}
    for tag, dt in DTYPES:
        got = ph.warp_image_forward(_cuda(im, dt), _cuda(flow, dt))
        assert got.dtype == dt and got.is_cuda and tuple(got.shape) == im.shape
        again = ph.warp_image_forward(_cuda(im, dt), _cuda(flow, dt))
        assert torch.equal(got.view(torch.int64 if dt == torch.float64 else torch.int32), again.view(torch.int64 if dt == torch.float64 else torch.int32))
        _bar(f"warp {tag}: {name}", got.cpu().numpy(), want["f64"], want["f32"], F64_FACTOR if tag == "f64" else 1.0)
    # numpy in, numpy float64 out; a CPU tensor stays a CPU tensor
    out = ph.warp_image_forward(im, flow)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == im.shape
    _bar(f"warp f64: {name} numpy", out, want["f64"], want["f32"], F64_FACTOR)
    cpu = ph.warp_image_forward(_t(im, torch.float32), _t(flow, torch.float32))
    assert not cpu.is_cuda and cpu.dtype == torch.float32


@pytest.mark.gpu
def test_warp_batch_shared_and_per_item():
    from event_based_bos_amd import photometric as ph

    H, W = 37, 70
    flows = np.stack([PC.flow(k, 40 + i, H, W) for i, k in enumerate(("smooth", "band", "far"))])
    images = np.stack([PC.image(50 + i, H, W, 255.0) for i in range(3)])
    for tag, dt in DTYPES:
        per = ph.warp_image_forward_batch(_cuda(images, dt), _cuda(flows, dt))
        shared = ph.warp_image_forward_batch(_cuda(images[1], dt), _cuda(flows, dt))
        u8 = ph.warp_image_forward_batch(_cuda(images.astype(np.uint8)), _cuda(flows, dt))
        for b in range(3):
            assert torch.equal(per[b], ph.warp_image_forward(_cuda(images[b], dt), _cuda(flows[b], dt)))      # the place in the batch
            assert torch.equal(shared[b], ph.warp_image_forward(_cuda(images[1], dt), _cuda(flows[b], dt)))
            assert torch.equal(u8[b], ph.warp_image_forward(_cuda(images[b].astype(np.uint8).astype(np.float64), dt), _cuda(flows[b], dt)))


@pytest.mark.gpu
def test_warp_zero_flow_returns_the_image():
    """33 x 65: the base grid i / 16 - 1, i / 32 - 1 is exact in float32, every sample position is the pixel itself and the warp
    returns the image bit for bit.  At other sizes the float32 grid puts the positions a few 2^-24 off the pixels (the reference's
    do the same) and the interior agrees to that: within the bar."""
    from event_based_bos_amd import photometric as ph

    for tag, dt in DTYPES:
        im = _cuda(PC.image(7, 33, 65, 255.0), dt)
        out = ph.warp_image_forward(im, torch.zeros(2, 33, 65, dtype=dt, device="cuda"))
        assert torch.equal(out[:-1, :-1], im[:-1, :-1]) and torch.equal(out, im)
        im = PC.image(8, 37, 70, 255.0)
        zero = np.zeros((2, 37, 70))
        want = {t: R.warp_forward(_t(im, d), _t(zero, d)).double().numpy() for t, d in DTYPES}
        out = ph.warp_image_forward(_cuda(im, dt), _cuda(zero, dt)).cpu().numpy()
        _bar(f"warp {tag}: zero flow 37x70", out, want["f64"], want["f32"], F64_FACTOR if tag == "f64" else 1.0)
        assert np.abs(out[1:-1, 1:-1] - im[1:-1, 1:-1]).max() < 255.0 * 70 * 2.0 ** -22


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PC.SHIFT_CASES))
def test_warp_image_torch(name):
    from event_based_bos_amd import photometric as ph

    im, shift = PC.shift_inputs(name)
    want = {tag: R.warp_shift(_t(im), _t(shift, dt)).numpy() for tag, dt in DTYPES}
    # r: the restatement run wholly in float32 (a constant float32 flow, a float32 image) against the float64 one
    all32 = R.warp_forward(_t(im, torch.float32), _t(shift, torch.float32)[:, None, None].expand(2, *im.shape).contiguous()).double().numpy()
    for tag, dt in DTYPES:
        got = ph.warp_image_torch(_cuda(im), _cuda(shift, dt))
        assert got.dtype == torch.float64 and got.is_cuda
        assert torch.equal(got, ph.warp_image_torch(_cuda(im), _cuda(shift, dt)))
        # both variants sample in float64: the float64 bar, around the restatement with the same shift dtype
        _bar(f"shift {tag}: {name}", got.cpu().numpy(), want[tag], all32 + (want[tag] - want["f64"]), F64_FACTOR)
    assert not ph.warp_image_torch(_t(im), _t(shift)).is_cuda


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PC.SSIM_CASES))
def test_ssim(name):
    from event_based_bos_amd import photometric as ph

    B, C, (H, W), _, ws = PC.SSIM_CASES[name]
    a, b = PC.ssim_inputs(name)
    maps = {tag: R.ssim_map(_t(a, dt), _t(b, dt), ws).double().numpy() for tag, dt in DTYPES}
    mean = {tag: R.ssim_mean(_t(a, dt), _t(b, dt), ws, True).double().numpy() for tag, dt in DTYPES}
    item = {tag: R.ssim_mean(_t(a, dt), _t(b, dt), ws, False).double().numpy() for tag, dt in DTYPES}
    for tag, dt in DTYPES:
        f = F64_FACTOR if tag == "f64" else 1.0
        x, y = _cuda(a, dt), _cuda(b, dt)
        got = ph.ssim_map(x, y, ws)
        assert got.dtype == dt and got.is_cuda and tuple(got.shape) == (B, C, H, W)
        assert torch.equal(got, ph.ssim_map(x, y, ws))
        _bar(f"ssim map {tag}: {name}", got.cpu().numpy(), maps["f64"], maps["f32"], f)
        m = ph.ssim(x, y, ws)
        assert m.dtype == dt and m.dim() == 0 and torch.equal(m, ph.ssim(x, y, ws, True)) and torch.equal(m, ph.SSIM(ws)(x, y))
        _bar(f"ssim mean {tag}: {name}", m.cpu().numpy(), mean["f64"], mean["f32"], f)
        per = ph.ssim(x, y, ws, size_average=False)
        assert per.dtype == dt and tuple(per.shape) == (B,) and torch.equal(per, ph.SSIM(ws, False).forward(x, y))
        _bar(f"ssim mean {tag}: {name} per item", per.cpu().numpy(), item["f64"], item["f32"], f)
        # an item's map and mean do not depend on its place in the batch
        if B > 1:
            assert torch.equal(ph.ssim_map(x[1:2], y[1:2], ws), got[1:2])
            assert torch.equal(ph.ssim(x[2:3], y[2:3], ws, False), per[2:3])
    assert not ph.ssim_map(_t(a), _t(b), ws).is_cuda


def _score_restatement(inp, dt, drop):
    B = inp["flow"].shape[0]
    rows = []
    for b in range(B):
        f1 = inp["frame1"] if inp["frame1"].ndim == 2 else inp["frame1"][b]
        rows.append(R.score(_t(f1, dt), _t(inp["frame2"][b], dt), _t(inp["flow"][b], dt), inp["roi"],
                            None if inp["mask"] is None else inp["mask"][b], window_size=inp["window_size"], drop=drop[b]))
    return torch.stack(rows).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PC.SCORE_CASES))
def test_photometric_error_batch(name):
    from event_based_bos_amd import photometric as ph

    (H, W), kinds, shared, *_rest = PC.SCORE_CASES[name]
    inp = PC.score_inputs(name)
    inp["window_size"] = ws = PC.SCORE_WINDOW.get(name, 11)
    B = len(kinds)
    # pixels within W 2^-22 of a tap boundary are left out of the comparison (through the mask, on both sides)
    drop = torch.stack([R.near_boundary(_t(inp["flow"][b]), W * 2.0 ** -22) if kinds[b] != "far" else torch.zeros(H, W, dtype=torch.bool)
                        for b in range(B)])
    assert int(drop.sum()) <= 1e-3 * H * W * B
    mask = inp["mask"]
    if drop.any():
        mask = (np.ones((B, H, W), np.uint8) if mask is None else mask) * (~drop.numpy())
    want = {tag: _score_restatement(inp, dt, drop) for tag, dt in DTYPES}
    for tag, dt in DTYPES:
        f1, f2, fl = _cuda(inp["frame1"], dt), _cuda(inp["frame2"], dt), _cuda(inp["flow"], dt)
        m = None if mask is None else _cuda(mask)
        table, cols = ph.photometric_error_batch(f1, f2, fl, roi=inp["roi"], mask=m, window_size=ws)
        assert cols == ph.COLUMNS and table.dtype == torch.float64 and table.is_cuda and tuple(table.shape) == (B, 7)
        again, _ = ph.photometric_error_batch(f1, f2, fl, roi=inp["roi"], mask=m, window_size=ws)
        assert torch.equal(table.view(torch.int64), again.view(torch.int64))
        got = table.cpu().numpy()
        print(f"{name} {tag} n_points {got[:, 6]} / {want['f64'][:, 6]}")
        assert np.array_equal(got[:, 6], want["f64"][:, 6]), (name, tag)
        for j, col in enumerate(ph.COLUMNS[:6]):
            _bar(f"score {col} {tag}: {name}", got[:, j], want["f64"][:, j], want["f32"][:, j], F64_FACTOR if tag == "f64" else 1.0)
        for b, kind in enumerate(kinds):
            if kind == "far":
                assert got[b, 6] == 0 and np.isnan(got[b, :6]).all()
        # an item's row does not depend on its place in the batch; one item through photometric_error
        order = list(range(B))[::-1]
        back, _ = ph.photometric_error_batch(f1 if shared else f1[order], f2[order], fl[order], roi=inp["roi"], mask=None if m is None else m[order],
                                              window_size=ws)
        assert torch.equal(back.view(torch.int64), table[order].view(torch.int64))
        one = ph.photometric_error(f1 if shared else f1[B - 1], f2[B - 1], fl[B - 1], roi=inp["roi"], mask=None if m is None else m[B - 1],
                                   window_size=ws)
        assert list(one) == list(ph.COLUMNS) and all(isinstance(v, np.float64) for v in one.values())
        assert np.array_equal(np.array(list(one.values())), got[B - 1], equal_nan=True)
    # numpy in: uploaded
    table, _ = ph.photometric_error_batch(inp["frame1"], inp["frame2"], inp["flow"], roi=inp["roi"], mask=mask, window_size=ws)
    assert table.is_cuda


@pytest.mark.gpu
def test_score_ssim_is_the_map_s_mean_over_the_counted_pixels():
    """The fused kernel evaluates the SSIM strip with the function of ``ssim_map``: its SSIM column is the float64 mean of that map
    over the counted pixels, to the last few bits of the sum."""
    from event_based_bos_amd import photometric as ph

    inp = PC.score_inputs("p_37x70_shared")
    f1, f2, fl = _cuda(inp["frame1"], torch.float32), _cuda(inp["frame2"], torch.float32), _cuda(inp["flow"], torch.float32)
    table, _ = ph.photometric_error_batch(f1, f2, fl)
    w = ph.warp_image_forward(f1, fl[0])
    ok = R.counted(fl[0].cpu()).cuda()
    q = ph.ssim_map(w[None, None], f2[None])[0, 0][ok].double()
    q0 = ph.ssim_map(f1[None, None], f2[None])[0, 0][ok].double()
    assert int(ok.sum()) == int(table[0, 6])
    assert abs(float(q.mean()) - float(table[0, 2])) < 1e-13 and abs(float(q0.mean()) - float(table[0, 5])) < 1e-13
    d = (w - f2[0])[ok]
    assert abs(float(d.abs().double().mean()) - float(table[0, 0])) < 1e-11 * 255


def _nan_filled(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("tag,dt", DTYPES)
def test_outputs_are_fully_written(tag, dt):
    """Every entry of the C ABI on NaN-filled outputs: no element is left as it was (37 x 70: partial tiles at both borders)."""
    from event_based_bos_amd import _hip, photometric as ph

    lib = _hip.require_gpu()
    H, W, B = 37, 70, 3
    code = _hip.IMAGE_F64 if dt == torch.float64 else _hip.IMAGE_F32
    images = _cuda(np.stack([PC.image(60 + b, H, W, 255.0) for b in range(B)]), dt)
    flows = _cuda(np.stack([PC.flow("smooth", 70 + b, H, W) for b in range(B)]), dt)
    s = _hip.stream_ptr(images.device)
    out = _nan_filled((B, H, W), dt)
    fn = lib.ebos_warp_image_forward_f64 if dt == torch.float64 else lib.ebos_warp_image_forward_f32
    _hip.check(fn(images.data_ptr(), code, H * W, flows.data_ptr(), None, 0, B, H, W, out.data_ptr(), s), "warp")
    assert not torch.isnan(out).any() and torch.equal(out, ph.warp_image_forward_batch(images, flows))
    taps = ph.window_taps(11, dt).cuda()
    maps, means = _nan_filled((B, 1, H, W), dt), _nan_filled((int(lib.ebos_ssim_means_elems(code, B, 1, H, W)),), torch.float64)
    fn = lib.ebos_ssim_map_f64 if dt == torch.float64 else lib.ebos_ssim_map_f32
    _hip.check(fn(out.data_ptr(), images.data_ptr(), taps.data_ptr(), 11, B, 1, H, W, maps.data_ptr(), means.data_ptr(), s), "ssim")
    assert not torch.isnan(maps).any() and not torch.isnan(means[:2 * B + 1]).any()
    assert torch.equal(means[B:2 * B].to(dt), ph.ssim(out[:, None], images[:, None], size_average=False))
    table = _nan_filled((B, 7), torch.float64)
    nbytes = lib.ebos_photometric_scratch_bytes(code, B, H, W)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    _hip.check(lib.ebos_photometric_batch(code, code, B, H, W, images.data_ptr(), H * W, images.roll(1, 0).contiguous().data_ptr(),
                                          flows.data_ptr(), taps.data_ptr(), 11, 0, 0, 0, 0, 0, None, 0, table.data_ptr(),
                                          scratch.data_ptr(), nbytes, s), "photometric")
    assert not torch.isnan(table).any() and (table[:, 6] > 0).all()


@pytest.mark.gpu
def test_orientation_on_the_synthetic_recording(tmp_path):
    """Frame f + d of ``evaluation.synthetic_recording`` is frame f sampled at x + d (0.6, 0.4) bump, so the flow that explains the
    pair is -d (0.6, 0.4) bump (rows first): it must score better than no flow, and its negative worse.  (The restatement gives, on
    the CPU, SSIM 0.9966 > 0.8883 > 0.7598 and L1 1.019 < 6.334 < 9.901 for frames 1 and 4 over the 5985 counted pixels.)"""
    from event_based_bos_amd import photometric as ph
    from event_based_bos_amd.evaluation import synthetic_recording

    H, W = 64, 96
    _, fr_path, _, _ = synthetic_recording(str(tmp_path), (H, W), 8, 100)
    frames = np.load(fr_path)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    bump = np.exp(-((yy - H / 2) ** 2 / (H / 4) ** 2 + (xx - W / 2) ** 2 / (W / 4) ** 2))
    for f, d in ((1, 3), (2, 4)):
        flow = np.stack([-d * 0.6 * bump, -d * 0.4 * bump]).astype(np.float32)
        good = ph.photometric_error(frames[f], frames[f + d], flow)
        bad = ph.photometric_error(frames[f], frames[f + d], -flow)
        print(f"frames {f}, {f + d}: SSIM {good['SSIM']:.4f} > {good['SSIM_0']:.4f} > {bad['SSIM']:.4f};  "
              f"L1 {good['L1']:.3f} < {good['L1_0']:.3f} < {bad['L1']:.3f}")
        assert good["SSIM"] > good["SSIM_0"] > bad["SSIM"]
        assert good["L1"] < good["L1_0"] < bad["L1"]
        assert good["n_points"] > 0.8 * H * W
