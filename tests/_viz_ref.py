"""A numpy restatement of the reference visualizer's pictures (src/visualizer.py, src/solver/base.py:154-287) and of the two OpenCV
calls they rest on: ``cv2.cvtColor(hsv, COLOR_HSV2RGB)`` on uint8 and ``cv2.morphologyEx(mask, MORPH_CLOSE, 3 x 3 MORPH_CROSS)``.

OpenCV is not installed where these tests run.  Like tests/_farneback_ref.py and tests/_warp_ref.py this file restates OpenCV's
algorithm (modules/imgproc: HSV2RGB_b around HSV2RGB_native, hue range 180; the morphology filters with their default border
values) and is NOT checked against OpenCV.  ``install_cv2_shim`` hands these two to the reference's own ``Visualizer`` so that
tests/golden/make_golden_viz.py can pin everything the wrapper does around them.

Two casts numpy leaves undefined are given a value here, the one x86 produces: a NaN angle (a NaN flow component) becomes hue 0,
and ``255 mag / max`` above 255 keeps its low byte.
"""
import sys
import types

import numpy as np

F = np.float32


# ------------------------------------------------------------------------------------------------ OpenCV, restated
def hsv2rgb_u8(hsv):
    """[..., 3] uint8 (H 0 - 180 nominal, any byte accepted) -> [..., 3] uint8 RGB."""
    hsv = np.asarray(hsv, dtype=np.uint8)
    h = hsv[..., 0].astype(F)
    s = hsv[..., 1].astype(F) * (F(1.0) / F(255.0))
    v = hsv[..., 2].astype(F) * (F(1.0) / F(255.0))
    h = h * (F(6.0) / F(180.0))
    h = np.fmod(h, F(6.0))
    sector = np.floor(h).astype(np.int32)
    h = h - sector.astype(F)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, F(0.0), h).astype(F)
    one = F(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1).astype(F)
    sector_data = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # (b, g, r)
    idx = sector_data[sector]
    b = np.take_along_axis(tab, idx[..., 0:1], axis=-1)[..., 0]
    g = np.take_along_axis(tab, idx[..., 1:2], axis=-1)[..., 0]
    r = np.take_along_axis(tab, idx[..., 2:3], axis=-1)[..., 0]
    grey = s == 0
    rgb = np.stack([np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)], axis=-1).astype(F)
    return np.clip(np.rint(rgb * F(255.0)), 0, 255).astype(np.uint8)


CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.uint8)


def _morph(img, element, dilate):
    H, W = img.shape
    fill = 0 if dilate else 255
    p = np.full((H + 2, W + 2), fill, dtype=np.uint8)
    p[1:-1, 1:-1] = img
    out = np.full((H, W), fill, dtype=np.uint8)
    for dr in range(3):
        for dc in range(3):
            if element[dr, dc]:
                nb = p[dr:dr + H, dc:dc + W]
                out = np.maximum(out, nb) if dilate else np.minimum(out, nb)
    return out


def mask_close(mask, element=CROSS):
    """MORPH_CLOSE = dilate then erode; outside pixels never win the dilation and never lose the erosion.  [H, W] -> uint8."""
    img = np.asarray(mask).astype(np.uint8)
    return _morph(_morph(img, element, True), element, False)


def install_cv2_shim():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_HSV2RGB, cv2.MORPH_CROSS, cv2.MORPH_CLOSE = 55, 1, 3

    def cvtColor(src, code):
        assert code == cv2.COLOR_HSV2RGB and src.dtype == np.uint8
        return hsv2rgb_u8(src)

    def getStructuringElement(shape, ksize, anchor=(-1, -1)):
        assert shape == cv2.MORPH_CROSS and tuple(ksize) == (3, 3) and tuple(anchor) in ((1, 1), (-1, -1))
        return CROSS.copy()

    def morphologyEx(src, op, kernel):
        assert op == cv2.MORPH_CLOSE and src.dtype == np.uint8 and src.ndim == 2
        return mask_close(src, kernel)

    cv2.cvtColor, cv2.getStructuringElement, cv2.morphologyEx = cvtColor, getStructuringElement, morphologyEx
    sys.modules["cv2"] = cv2
    return cv2


# ------------------------------------------------------------------------------------------------ the visualizer, restated
def trunc_u8(v):
    """``.astype(np.uint8)`` of doubles as x86 computes it: towards zero, low byte, NaN -> 0."""
    v = np.asarray(v, dtype=np.float64)
    return (np.where(np.isfinite(v), v, 0.0).astype(np.int64) & 0xFF).astype(np.uint8)


def magnitude(fx, fy, ord):
    flows = np.stack((fx, fy), axis=2).astype(np.float64)
    flows[np.isinf(flows)] = 0
    flows[np.isnan(flows)] = 0
    return np.linalg.norm(flows, axis=2) ** ord


def flow_hsv_doubles(fx, fy, max_magnitude=None, ord=1.0):
    """-> (ang, 255 mag / max, max): the doubles color_optical_flow truncates to hue and value."""
    fx, fy = np.asarray(fx, dtype=np.float64), np.asarray(fy, dtype=np.float64)
    mag = magnitude(fx, fy, ord)
    with np.errstate(all="ignore"):
        ang = (np.arctan2(fy, fx) + np.pi) * 180.0 / np.pi / 2.0
        if max_magnitude is None:
            max_magnitude = mag.max()
        val = 255 * mag / max_magnitude if max_magnitude > 0 else np.zeros_like(mag)   # (an all-zero flow: black, the package's rule)
    return ang, val, max_magnitude


def color_optical_flow(fx, fy, max_magnitude=None, ord=1.0):
    """-> (flow_rgb [H, W, 3], color_wheel [H, H, 3], max_magnitude)."""
    ang, val, max_magnitude = flow_hsv_doubles(fx, fy, max_magnitude, ord)
    hsv = np.zeros(ang.shape + (3,), dtype=np.uint8)
    hsv[..., 0], hsv[..., 1], hsv[..., 2] = trunc_u8(ang), 255, trunc_u8(val)
    return hsv2rgb_u8(hsv), color_wheel(ang.shape[0]), max_magnitude


def color_wheel(H):
    xx, yy = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, H))
    mag = np.linalg.norm(np.stack((xx, yy), axis=2), axis=2)
    ang = (np.arctan2(yy, xx) + np.pi) * 180 / np.pi / 2.0
    hsv = np.zeros((H, H, 3), dtype=np.uint8)
    hsv[..., 0], hsv[..., 1], hsv[..., 2] = trunc_u8(ang), 255, trunc_u8(255 * mag / mag.max())
    return hsv2rgb_u8(hsv)


def flow_on_event_mask(flow, mask, ord=0.5, max_color_on_mask=True, mask_color="white", mask_morph=False):
    """visualize_optical_flow_on_event_mask with the event mask given ([H, W] bool) -> [H, W, 3]."""
    mask = np.asarray(mask).astype(bool)
    if mask_morph:
        mask = mask_close(mask.astype(np.uint8)).astype(bool)
    used = flow * mask[None] if max_color_on_mask else flow
    rgb = color_optical_flow(used[0], used[1], ord=ord)[0].copy()
    rgb[~mask] = 255 if mask_color == "white" else 0
    return rgb


def pred_and_gt(pred, gt, ord=0.5):
    m = max(color_optical_flow(pred[0], pred[1], ord=ord)[2], color_optical_flow(gt[0], gt[1], ord=ord)[2])
    return color_optical_flow(pred[0], pred[1], m, ord=ord)[0], color_optical_flow(gt[0], gt[1], m, ord=ord)[0]


def signed_counts(events, shape):
    """(n+, n-) [H, W] of ``visualize_event``: coordinates clipped into the image and truncated; polarity 0 / 1 or -1 / +1."""
    H, W = shape
    pos, neg = np.zeros((H, W)), np.zeros((H, W))
    if len(events):
        x = np.clip(events[:, 0], 0, H - 1).astype(np.int32)
        y = np.clip(events[:, 1], 0, W - 1).astype(np.int32)
        pol = events[:, 3] * 2 - 1 if np.min(events[:, 3]) == 0 else events[:, 3]
        np.add.at(pos, (x[pol > 0], y[pol > 0]), 1)
        np.add.at(neg, (x[pol < 0], y[pol < 0]), 1)
    return pos, neg


def event_picture(pos, neg, background_color=127):
    return np.clip((pos - neg) * 20 + background_color, 0, 255).astype(np.uint8)


def clipped_iwe(iwe, max_scale=50, pad=0):
    out = 255 - np.clip(max_scale * np.asarray(iwe, dtype=np.float64), 0, 255).astype(np.uint8)
    return out[pad:-pad, pad:-pad] if pad > 0 else out


def centered_double(a):
    """standardize_image_center(a) before the cast (an all-zero field: 128, the package's rule)."""
    a = np.asarray(a, dtype=np.float64)
    m = np.abs(a).max()
    return a / m * 127 + 128 if m > 0 else np.full_like(a, 128.0)


def centered(a):
    return trunc_u8(centered_double(a))


def integer_iwe(events, shape):
    """The bilinear vote of integer-pixel events inside the image: the events per pixel."""
    pos, neg = np.zeros(shape), np.zeros(shape)
    np.add.at(pos, (events[:, 0].astype(int), events[:, 1].astype(int)), 1)
    return pos + neg


def step_pictures(orig_events, filter_events, pred, gt, shape, poisson_pred, poisson_gt, pad=0, max_scale=50):
    """The ten pictures of one driver step (bos_event.py:202-207) from integer-pixel events, the two flows [2, H, W] and the two
    Poisson fields [H, W] that ``visualize_poisson_integration`` standardises."""
    mask = integer_iwe(filter_events, shape) != 0
    cmp_pred, cmp_gt = pred_and_gt(pred, gt)
    return {
        "original": event_picture(*signed_counts(orig_events, shape)),
        "original_filter": clipped_iwe(integer_iwe(filter_events, shape), max_scale, pad),
        "flow_comparison_pred": cmp_pred,
        "flow_comparison_gt": cmp_gt,
        "pred_flow": color_optical_flow(pred[0], pred[1], ord=0.5)[0],
        "pred_flow_poisson": centered(poisson_pred),
        "pred_masked": flow_on_event_mask(pred, mask, mask_color="black", mask_morph=True),
        "gt_flow": color_optical_flow(gt[0], gt[1], ord=0.5)[0],
        "gt_flow_poisson": centered(poisson_gt),
        "gt_masked": flow_on_event_mask(gt, mask, mask_color="black", mask_morph=True),
    }


PICTURES = ("original", "original_filter", "flow_comparison_pred", "flow_comparison_gt", "pred_flow", "pred_flow_poisson",
            "pred_masked", "gt_flow", "gt_flow_poisson", "gt_masked")


def kink_free(*doubles, margin=1e-6):
    """True where none of the pre-truncation doubles lies within ``margin`` of an integer (NaN counts as free: its cast is fixed)."""
    ok = np.ones(np.shape(doubles[0]), dtype=bool)
    for d in doubles:
        d = np.asarray(d, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            near = np.abs(d - np.rint(d)) < margin
        ok &= ~(near & np.isfinite(d))
    return ok


def comparable(ang, val, margin=1e-6):
    """The pixels of a colour picture a device whose atan2 / sqrt differ from libm in the last bit must reproduce: value and hue
    doubles off the integers -- but a value below 0.5 truncates to 0 whatever its last bit, and a black pixel has no hue."""
    with np.errstate(invalid="ignore"):
        v_ok = kink_free(val, margin=margin) | (np.asarray(val) < 0.5)
    return v_ok & (kink_free(ang, margin=margin) | (trunc_u8(val) == 0))


def centered_comparable(a, margin=1e-6):
    """The pixels of a centred picture to compare: off the integers, or an exact zero of the field (the boundary of a Poisson
    field), which is 128 in any IEEE arithmetic."""
    a = np.asarray(a, dtype=np.float64)
    return kink_free(centered_double(a), margin=margin) | (a == 0)
