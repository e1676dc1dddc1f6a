"""Seeded cases of tests/golden/golden_farneback.npz (tests/golden/make_golden_farneback.py).  Frames are built with integer
arithmetic only, so every machine rebuilds the same bits: a smooth uint8 texture drawn at twice the resolution, averaged 2 x 2, and
the same texture moved by a few half-pixels (a uniform part plus a bump in the middle) for the later frames."""
import numpy as np

YAML = {"pyr_scale": 0.5, "levels": 4, "winsize": 10, "iterations": 3, "poly_n": 5, "poly_sigma": 1.2, "flags": 0}

# name: frame shape, ROI (rows x0:x1, columns y0:y1) or None, dtype, params, method, stored rows step
CASES = {
    "roi_yaml_u8": dict(shape=(96, 160), roi=(8, 88, 32, 128), dtype=np.uint8, params=YAML, method="opencv_flow", seed=1),
    "odd65x87_f32": dict(shape=(65, 87), roi=None, dtype=np.float32, method="opencv_flow", seed=2,
                         params=dict(YAML, levels=2, winsize=9, iterations=2, poly_sigma=1.1)),
    "s260x346_u8": dict(shape=(260, 346), roi=None, dtype=np.uint8, params=YAML, method="opencv_flow", seed=3, row_step=4),
    "pyr08_f64": dict(shape=(72, 90), roi=None, dtype=np.float64, method="opencv_flow", seed=4,
                      params=dict(YAML, pyr_scale=0.8, levels=5, winsize=7, poly_n=7, poly_sigma=1.5)),
    "win1_it1_u8": dict(shape=(48, 64), roi=None, dtype=np.uint8, method="opencv_flow", seed=5,
                        params=dict(YAML, levels=2, winsize=1, iterations=1, poly_sigma=1.1)),
    "twostep_roi_u8": dict(shape=(64, 80), roi=(0, 64, 8, 72), dtype=np.uint8, params=YAML, method="opencv_flow_two_steps", seed=6),
    "twostep_p7_u8": dict(shape=(48, 56), roi=None, dtype=np.uint8, method="opencv_flow_two_steps", seed=7,
                          params=dict(YAML, winsize=5, poly_n=7, poly_sigma=1.5)),
}


def _texture(rng, H, W):
    """A smooth uint8-range int64 texture [H, W]: a 9 x 9 box sum of random integers, rescaled with integer division."""
    r = rng.integers(0, 256, size=(H + 8, W + 8), dtype=np.int64)
    c = np.cumsum(np.cumsum(np.pad(r, ((1, 0), (1, 0))), 0), 1)
    s = c[9:, 9:] - c[:-9, 9:] - c[9:, :-9] + c[:-9, :-9]
    s = s - s.min()
    return s * 255 // max(int(s.max()), 1)


def _moved(T, sy, sx):
    """T [2H + 16, 2W + 16] sampled at rows 8 + 2 i - sy(i, j), columns 8 + 2 j - sx(i, j) (integer half-pixel steps) and averaged
    2 x 2 -> [H, W]."""
    H2, W2 = T.shape[0] - 16, T.shape[1] - 16
    ii, jj = np.meshgrid(np.arange(H2), np.arange(W2), indexing="ij")
    v = T[8 + ii - sy[ii // 2, jj // 2], 8 + jj - sx[ii // 2, jj // 2]]
    return (v[0::2, 0::2] + v[1::2, 0::2] + v[0::2, 1::2] + v[1::2, 1::2] + 2) // 4


def _shift_field(H, W, amp):
    """Integer half-pixel displacement: `amp` everywhere plus one more inside a centred box."""
    s = np.full((H, W), amp, dtype=np.int64)
    s[H // 4:3 * H // 4, W // 4:3 * W // 4] += 1
    return s


def _as_dtype(u, dtype):
    if dtype == np.uint8:
        return u.astype(np.uint8)
    return u.astype(dtype) * dtype(0.5) + dtype(3)      # exact in float32 and float64


def case_frames(name):
    """-> (frame0, frame1, frame2): full-size frames of the case's dtype.  frame1 -> frame2 moves by (1 + bump, 2 + bump) half
    pixels; frame0 (the background of the two-step method) lies two half pixels before frame1."""
    c = CASES[name]
    H, W = c["shape"]
    rng = np.random.default_rng(c["seed"])
    T = _texture(rng, 2 * H + 16, 2 * W + 16)
    zero = np.zeros((H, W), dtype=np.int64)
    f0 = _moved(T, zero, zero)
    f1 = _moved(T, _shift_field(H, W, 1), zero + 1)
    f2 = _moved(T, _shift_field(H, W, 2), _shift_field(H, W, 3))
    return tuple(_as_dtype(f, c["dtype"]) for f in (f0, f1, f2))


def crop(frame, roi):
    """bos_event.py validate_image: frame[..., xmin:xmax, ymin:ymax] (a view)."""
    if roi is None:
        return frame
    x0, x1, y0, y1 = roi
    return frame[..., x0:x1, y0:y1]


def case_config(name):
    """The propagated config the driver hands to FrameFlowEstimator.estimate: params_opencv_flow with the pad_* margins."""
    c = CASES[name]
    H, W = c["shape"]
    x0, x1, y0, y1 = c["roi"] or (0, H, 0, W)
    params = dict(c["params"], pad_x0=x0, pad_x1=H - x1, pad_y0=y0, pad_y1=W - y1)
    return {"method": c["method"], "params_opencv_flow": params}


def stored_rows(name):
    """Rows of the [2, H, W] result the fixture keeps."""
    return slice(None, None, CASES[name].get("row_step", 1))
