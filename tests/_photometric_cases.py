"""Seeded inputs of the photometric tests (tests/test_photometric.py) and of tests/golden/make_golden_photometric.py: the smallest
shapes at which the kernels of csrc/photometric.hip can still go wrong.

  7 x 9    smaller than the 11 x 11 window: padding everywhere, one partial tile
  23 x 19  one partial tile, more than one row of waves
  33 x 65  one pixel past a 32-column (float64 tile) and a 64-column (float32 tile) seam and past two 16-row seams; its base grid
           i / ((size - 1) / 2) - 1 is exact in float32 (16 and 32 are powers of two)
  37 x 70  several tiles in both directions, none of them whole at the border

Images are a seeded random field smoothed 3 x 3, so that no window is flat: on a flat window at range 255 the reference's own SSIM
ratio is ill-conditioned (sigma = E[x x] - mu mu cancels to rounding noise) and proves nothing.  Everything is built in float64 (or
uint8); the float32 variant of a case is the same arrays cast.
"""
import numpy as np

SHAPES = ((7, 9), (23, 19), (33, 65), (37, 70))


def image(seed, H, W, scale=1.0, uint8=False):
    """[H, W]: rand smoothed 3 x 3, float64 in [0, scale] or uint8 in [0, 255]."""
    a = np.random.RandomState(seed).rand(H + 2, W + 2)
    s = sum(a[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    if uint8:
        return np.round(s * 255.0).astype(np.uint8)
    return s * float(scale)


FLOW_KINDS = ("smooth", "band", "far", "nonfinite")


def flow(kind, seed, H, W):
    """[2, H, W] float64, rows first.  smooth: sub-pixel, low frequency; band: + 8 px on columns 2 .. 5, which pushes their taps
    outside (the image is sampled at x - flow); far: 1e6 everywhere, nothing is counted; nonfinite: a NaN and an inf."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    p, a = rs.uniform(0, 2 * np.pi, 4), rs.uniform(0.3, 0.9, 2)
    f = np.stack([a[0] * np.sin(2 * np.pi * yy / H + p[0]) * np.cos(2 * np.pi * xx / W + p[1]) + 0.31,
                  a[1] * np.cos(2 * np.pi * yy / H + p[2]) * np.sin(2 * np.pi * xx / W + p[3]) - 0.27])
    if kind == "band":
        f[1][:, 2:6] += 8.0
    elif kind == "far":
        f[:] = 1e6
    elif kind == "nonfinite":
        f[0, H // 2, W // 3] = np.nan
        f[1, H // 3, W // 2] = np.inf
    elif kind != "smooth":
        raise KeyError(kind)
    return f


# ---- the warp alone: name -> (shape, flow kind, image: "float" | "uint8", value range)
WARP_CASES = {
    "w_7x9_smooth": ((7, 9), "smooth", "float", 1.0),
    "w_23x19_band": ((23, 19), "band", "float", 255.0),
    "w_23x19_nonfinite": ((23, 19), "nonfinite", "float", 1.0),
    "w_23x19_uint8": ((23, 19), "smooth", "uint8", 255.0),
    "w_33x65_smooth": ((33, 65), "smooth", "float", 255.0),
    "w_37x70_band": ((37, 70), "band", "uint8", 255.0),
    "w_37x70_far": ((37, 70), "far", "float", 1.0),
}
GOLDEN_WARP = ("w_7x9_smooth", "w_23x19_band", "w_23x19_nonfinite", "w_23x19_uint8", "w_33x65_smooth")   # (the file stays small)
GOLDEN_WARP_NUMPY = ("w_7x9_smooth", "w_23x19_uint8")     # also through the reference's numpy path
GOLDEN_WARP_F64_ONLY = ("w_33x65_smooth",)


def warp_inputs(name):
    (H, W), kind, im, scale = WARP_CASES[name]
    seed = sorted(WARP_CASES).index(name)
    return image(100 + seed, H, W, scale, uint8=(im == "uint8")), flow(kind, 200 + seed, H, W)


# ---- warp_image_torch: name -> (shape, [2] shift): integer and half-pixel values
SHIFT_CASES = {
    "s_7x9": ((7, 9), (1.0, -2.0)),
    "s_23x19_half": ((23, 19), (0.5, 1.5)),
    "s_17x33_mixed": ((17, 33), (-3.0, 0.5)),
    "s_23x19_out": ((23, 19), (30.0, 0.0)),
}


def shift_inputs(name):
    (H, W), shift = SHIFT_CASES[name]
    return image(300 + sorted(SHIFT_CASES).index(name), H, W, 255.0), np.array(shift, dtype=np.float64)


# ---- SSIM: name -> (B, C, shape, value range, window size)
SSIM_CASES = {
    "q_1x1_7x9": (1, 1, (7, 9), 1.0, 11),
    "q_3x2_23x19": (3, 2, (23, 19), 255.0, 11),
    "q_1x2_33x65": (1, 2, (33, 65), 1.0, 11),
    "q_3x1_37x70": (3, 1, (37, 70), 255.0, 11),
    "q_1x1_23x19_w5": (1, 1, (23, 19), 255.0, 5),
    "q_1x1_33x65_w13": (1, 1, (33, 65), 1.0, 13),
}


def ssim_inputs(name):
    """(img1, img2) [B, C, H, W] float64: img2 = img1 displaced a little plus a second field, so that the map is neither 1 nor noise."""
    B, C, (H, W), scale, _ = SSIM_CASES[name]
    seed = 400 + 10 * sorted(SSIM_CASES).index(name)
    a = np.stack([image(seed + n, H, W + 1, scale) for n in range(B * C)]).reshape(B, C, H, W + 1)
    b = np.stack([image(seed + 50 + n, H, W, scale) for n in range(B * C)]).reshape(B, C, H, W)
    return np.ascontiguousarray(a[..., :W]), 0.7 * a[..., 1:] + 0.3 * b


# ---- the fused score: name -> (shape, flow kind per item, frame1 shared, frames: "float" | "uint8", value range, roi, with mask)
SCORE_CASES = {
    "p_7x9": ((7, 9), ("smooth",), False, "float", 1.0, None, False),
    "p_23x19_shared_u8": ((23, 19), ("smooth", "band", "far"), True, "uint8", 255.0, (2, 20, 1, 17), True),
    "p_33x65_f255": ((33, 65), ("band", "smooth", "nonfinite"), False, "float", 255.0, None, False),
    "p_37x70_u8": ((37, 70), ("smooth", "far", "band"), False, "uint8", 255.0, (3, 35, 4, 69), True),
    "p_37x70_shared": ((37, 70), ("smooth",), True, "float", 255.0, None, False),
    "p_33x65_shared_roi": ((33, 65), ("nonfinite", "band", "smooth"), True, "float", 1.0, (0, 33, 5, 60), True),
    "p_23x19_w5": ((23, 19), ("nonfinite", "smooth"), False, "float", 255.0, None, False),
    "p_37x70_w13": ((37, 70), ("band",), False, "uint8", 255.0, (1, 36, 0, 70), False),
}
SCORE_WINDOW = {"p_23x19_w5": 5, "p_37x70_w13": 13}   # (every other case: the default 11, which has kernels of its own)


def score_inputs(name):
    """-> dict(frame1 [H, W] or [B, H, W], frame2 [B, H, W], flow [B, 2, H, W] float64, roi, mask [B, H, W] uint8 or None).  frame2 of
    an item is frame1 displaced by about its smooth flow, plus a little of another field."""
    (H, W), kinds, shared, fr, scale, roi, with_mask = SCORE_CASES[name]
    seed = 500 + 20 * sorted(SCORE_CASES).index(name)
    u8, B = fr == "uint8", len(kinds)
    f1 = image(seed, H, W, scale, u8) if shared else np.stack([image(seed + b, H, W, scale, u8) for b in range(B)])
    flows = np.stack([flow(k, seed + 7 + b, H, W) for b, k in enumerate(kinds)])
    f2 = []
    for b in range(B):
        src = (f1 if shared else f1[b]).astype(np.float64)
        other = image(seed + 11 + b, H, W, 255.0 if u8 else scale)
        mix = 0.8 * np.roll(src, (0, 1), axis=(0, 1)) + 0.2 * other
        f2.append(np.round(mix).astype(np.uint8) if u8 else mix)
    mask = None
    if with_mask:
        mask = (np.random.RandomState(seed + 3).rand(B, H, W) > 0.3).astype(np.uint8) * 7   # (any non-zero value counts)
    return dict(frame1=f1, frame2=np.stack(f2), flow=flows, roi=roi, mask=mask)
