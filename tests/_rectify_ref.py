"""numpy restatement of csrc/rectify.hip: the lens model, its inverse iteration, event rectification, the reference's
``undistort_events`` and the fused image rectification, with the kernels' operation order (float64, every product and sum rounded on
its own), so a kernel built without fused multiply-adds agrees with it bit for bit.

The model (K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]], cx / fx on the COLUMN axis; D = (k1, k2, p1, p2[, k3[, k4, k5, k6]])):

    r2 = x*x + y*y;  rad = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2);  a = (2*x)*y
    dx = p1*a + p2*(r2 + 2*(x*x));  dy = p1*(r2 + 2*(y*y)) + p2*a;  u = fx*(x*rad + dx) + cx;  v = fy*(y*rad + dy) + cy

What this is not: it is not checked against OpenCV (``cv2.undistort``, ``cv2.initUndistortRectifyMap``), which is absent where this
package is developed.  The image path is checked against this restatement and against the forward model.
"""
import os

import numpy as np

import _warp_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_rectify.npz")

# the issue's cases: asymmetric on purpose, so that a row / column swap cannot pass
CASES = {
    "A": dict(size=(37, 70), f=(60.0, 57.0), c=(34.8, 17.6), D=(-0.25, 0.08, 1e-3, -5e-4, -0.01)),                  # barrel
    "B": dict(size=(64, 96), f=(80.0, 83.0), c=(47.8, 31.1), D=(0.12, -0.03, -8e-4, 6e-4, 0.004)),                  # pincushion
    "C": dict(size=(64, 96), f=(80.0, 83.0), c=(47.8, 31.1), D=(0.12, -0.03, -8e-4, 6e-4, 0.004, 0.02, -0.01, 0.003)),
}


def case_K(name):
    c = CASES[name]
    return np.array([[c["f"][0], 0.0, c["c"][0]], [0.0, c["f"][1], c["c"][1]], [0.0, 0.0, 1.0]])


def coefficients(D):
    d = np.zeros(8)
    d[:len(D)] = np.asarray(D, dtype=np.float64)
    return d


def lens_terms(D, x, y):
    """-> (rad, dx, dy) at the normalised points (x, y)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(D)
    xx, yy = x * x, y * y
    r2 = xx + yy
    rad = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
    a = (2.0 * x) * y
    return rad, p1 * a + p2 * (r2 + 2.0 * xx), p1 * (r2 + 2.0 * yy) + p2 * a


def forward_normalised(K, D, x, y):
    """Ideal normalised (x, y) -> sensor pixel (u = column, v = row)."""
    rad, dx, dy = lens_terms(D, x, y)
    return K[0, 0] * (x * rad + dx) + K[0, 2], K[1, 1] * (y * rad + dy) + K[1, 2]


def distort_points(K, D, points, new_K=None):
    """Rectified (row', col') under new_K -> sensor (row, col)."""
    nK = K if new_K is None else new_K
    p = np.asarray(points, dtype=np.float64)
    u, v = forward_normalised(K, D, (p[..., 1] - nK[0, 2]) / nK[0, 0], (p[..., 0] - nK[1, 2]) / nK[1, 1])
    return np.stack([v, u], axis=-1)


def inverse_points(K, D, points, new_K=None, iterations=20):
    """Sensor (row, col) -> rectified (row', col') under new_K: the fixed-count fixed-point iteration."""
    nK = K if new_K is None else new_K
    p = np.asarray(points, dtype=np.float64)
    x0, y0 = (p[..., 1] - K[0, 2]) / K[0, 0], (p[..., 0] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iterations):
        rad, dx, dy = lens_terms(D, x, y)
        x, y = (x0 - dx) / rad, (y0 - dy) / rad
    return np.stack([nK[1, 1] * y + nK[1, 2], nK[0, 0] * x + nK[0, 2]], axis=-1)


def pixel_grid(H, W):
    """[H, W, 2] float64 = (row, col)."""
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([r, c], axis=-1)


def rectify_map(K, D, sensor_size, new_K=None, iterations=20):
    return inverse_points(K, D, pixel_grid(*sensor_size), new_K, iterations)


def rectify_events_raw(col, row, t, pol, rmap, ticks_per_second=1e6, dtype=np.float64, image_size=None):
    """A gather on the map ``rmap`` [H, W, 2], the keep rule, the time conversion of ``RawEventStore.load_event``.
    -> (events [m, 4] of dtype, n_outside_sensor, n_outside_image)."""
    H, W = rmap.shape[:2]
    Ho, Wo = (H, W) if image_size is None else image_size
    col, row = np.asarray(col).astype(np.int64), np.asarray(row).astype(np.int64)
    inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    pos = rmap[np.where(inside, row, 0), np.where(inside, col, 0)].astype(dtype)
    with np.errstate(invalid="ignore"):
        in_image = (pos[:, 0] >= 0) & (pos[:, 0] < dtype(Ho)) & (pos[:, 1] >= 0) & (pos[:, 1] < dtype(Wo))
    keep = inside & in_image
    ev = np.zeros((len(col), 4), dtype=np.float64)
    ev[:, 2] = np.asarray(t) / ticks_per_second
    ev[:, 3] = np.asarray(pol) != 0
    ev = ev.astype(dtype)
    ev[:, :2] = pos
    return ev[keep], int((~inside).sum()), int((inside & ~in_image).sum())


def undistort_events(events, map_x, map_y, h, w):
    """The reference's function (src/utils/event_utils.py:261-266), restated."""
    k = np.int32(map_y[events[:, 0].astype(np.int32), events[:, 1].astype(np.int32)])
    l = np.int32(map_x[events[:, 0].astype(np.int32), events[:, 1].astype(np.int32)])  # noqa: E741
    out = np.copy(events)
    out[:, 0] = k
    out[:, 1] = l
    return out[((0 <= k) & (k < h)) & ((0 <= l) & (l < w))]


def has_lens(K, D, new_K=None):
    return bool(np.any(np.asarray(D) != 0) or (new_K is not None and np.any(np.asarray(new_K) != np.asarray(K))))


def image_coordinates(K, D, dsize, new_K=None, homography=None, rows=None, cols=None):
    """The float64 source position (u = column, v = row) [h, w] of destination rows ``rows`` and columns ``cols`` BEFORE the
    fixed-point rounding, by the kernel's lens chain: the perspective walk of _warp_ref.coordinates with the scale 1 / W, normalised
    by new_K, pushed through the forward model."""
    nK = K if new_K is None else new_K
    Wd_, Hd_ = int(dsize[0]), int(dsize[1])
    m = (np.eye(3) if homography is None else W.invert3x3(homography)).reshape(9)
    bw = W.block_width(Hd_, Wd_)
    x = np.arange(Wd_, dtype=np.int64) if cols is None else np.asarray(cols, dtype=np.int64)
    y = np.arange(Hd_, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    x0 = ((x // bw) * bw).astype(np.float64)[None, :]
    x1 = (x % bw).astype(np.float64)[None, :]
    yy = y.astype(np.float64)[:, None]
    X0 = (m[0] * x0 + m[1] * yy) + m[2]
    Y0 = (m[3] * x0 + m[4] * yy) + m[5]
    W0 = (m[6] * x0 + m[7] * yy) + m[8]
    Wd = W0 + m[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.where(Wd != 0, 1.0 / np.where(Wd != 0, Wd, 1.0), 0.0)
        xn = ((X0 + m[0] * x1) * s - nK[0, 2]) / nK[0, 0]
        yn = ((Y0 + m[3] * x1) * s - nK[1, 2]) / nK[1, 1]
        return forward_normalised(K, D, xn, yn)


def sample(src, X, Y, border_value=0):
    """The INTER_LINEAR sampling of _warp_ref.warp_perspective at the integer coordinates (X, Y) (scaled by 32)."""
    src = np.asarray(src)
    Hs, Ws = src.shape
    cval = W.border_as(src.dtype, border_value)

    def tap(sy, sx):
        inside = (sx >= 0) & (sx < Ws) & (sy >= 0) & (sy < Hs)
        v = src[np.clip(sy, 0, Hs - 1), np.clip(sx, 0, Ws - 1)]
        return np.where(inside, v, cval).astype(src.dtype), inside

    sx, sy = W._sat16(X >> W.INTER_BITS), W._sat16(Y >> W.INTER_BITS)
    fx, fy = X & (W.INTER_TAB_SIZE - 1), Y & (W.INTER_TAB_SIZE - 1)
    (s00, i00), (s01, i01), (s10, i10), (s11, i11) = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    none_inside = ~(i00 | i01 | i10 | i11)
    if src.dtype == np.uint8:
        w = W.interp_table()[fy, fx]
        acc = s00.astype(np.int64) * w[..., 0, 0] + s01.astype(np.int64) * w[..., 0, 1] + s10.astype(np.int64) * w[..., 1, 0] \
            + s11.astype(np.int64) * w[..., 1, 1]
        out = np.clip((acc + (1 << (W.COEF_BITS - 1))) >> W.COEF_BITS, 0, 255).astype(np.uint8)
    else:
        step = np.float32(1.0 / W.INTER_TAB_SIZE)
        bx, by = fx.astype(np.float32) * step, fy.astype(np.float32) * step
        ax, ay = np.float32(1) - bx, np.float32(1) - by
        out = ((s00 * (ay * ax) + s01 * (ay * bx)) + s10 * (by * ax)) + s11 * (by * bx)
    return np.where(none_inside, cval, out).astype(src.dtype)


def undistort_image(src, K, D, new_K=None, homography=None, dsize=None, roi=None, border_value=0):
    """src [Hs, Ws] uint8 | float32 -> the rectified frame [H, W] (dsize = (W, H), default the source's) or its ``roi`` rows
    [xmin, xmax) and columns [ymin, ymax).  ``homography``: ideal frame -> destination, as cv2.warpPerspective takes it.  ONE
    resample: this is not ``warp_perspective(undistort(src))``, which resamples twice."""
    src = np.asarray(src)
    Wd, Hd = (src.shape[1], src.shape[0]) if dsize is None else (int(dsize[0]), int(dsize[1]))
    if not has_lens(K, D, new_K):
        return W.warp_perspective(src, np.eye(3) if homography is None else homography, (Wd, Hd), W.INTER_LINEAR, border_value, roi)
    xmin, xmax, ymin, ymax = (0, Hd, 0, Wd) if roi is None else (int(v) for v in roi)
    u, v = image_coordinates(K, D, (Wd, Hd), new_K, homography, np.arange(xmin, xmax), np.arange(ymin, ymax))
    with np.errstate(over="ignore", invalid="ignore"):
        fX = np.fmax(float(W.INT_MIN), np.fmin(float(W.INT_MAX), u * float(W.INTER_TAB_SIZE)))
        fY = np.fmax(float(W.INT_MIN), np.fmin(float(W.INT_MAX), v * float(W.INTER_TAB_SIZE)))
    return sample(src, np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64), border_value)


# ---- the fixture made by the reference's undistort_events (tests/golden/make_golden_rectify.py)
def golden_sets():
    """name -> (events float64, map_x, map_y, h, w, {dtype tag: (kept rows, their (k, l))})."""
    g = np.load(GOLDEN)
    H, W = CASES["A"]["size"]
    rmap = rectify_map(case_K("A"), CASES["A"]["D"], (H, W))
    assert np.array_equal(np.array([rmap[..., 0].sum(), rmap[..., 1].sum()]), g["lens_map_sum"]), "the maps are not the generator's"
    maps = {"lens": (np.ascontiguousarray(rmap[..., 1]), np.ascontiguousarray(rmap[..., 0])), "small": (g["small_map_x"], g["small_map_y"])}
    return {name: (g[f"{name}_events"], maps[name][0], maps[name][1], int(g[f"{name}_hw"][0]), int(g[f"{name}_hw"][1]),
                   {tag: (g[f"{name}_{tag}_idx"], g[f"{name}_{tag}_kl"]) for tag in ("f64", "f32")}) for name in ("lens", "small")}


def golden_output(events, idx, kl):
    want = events[idx].copy()
    want[:, :2] = kl
    return want
