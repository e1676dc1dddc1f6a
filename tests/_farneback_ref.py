"""A numpy restatement of OpenCV's ``cv2.calcOpticalFlowFarneback`` (CPU path, flags 0), the form csrc/farneback.hip computes.

OpenCV is not available where this project is developed, so this file is written from the published algorithm (Farneback 2003) and
OpenCV 4.x's ``optflowgf.cpp`` as its structure is documented; the analytic tests in tests/test_frame_flow.py (an exact quadratic
through the polynomial expansion, a known sub-pixel shift through the whole estimator) hold it to the maths.  It is the
definition the GPU kernels are checked against; bit-level agreement with OpenCV itself is not checked anywhere.

Precision follows OpenCV's storage: images, the expansion R, the matrices M and the flow are float32; the horizontal pass of the
expansion and the window sums of M are float64.  Every float32 operation below is one IEEE operation in a fixed order (numpy does
not contract a * b + c), and the kernels perform the same operations in the same order.

Deliberate choices where OpenCV's source could not be consulted:
  - the exact 2x downscale uses the INTER_LINEAR formula (weights 1/2, 1/2), the same 2 x 2 mean as INTER_AREA up to the order of
    the float32 additions;
  - the (2m+1)^2 window sum is the plain replicate-border box sum, also for winsize 1.
"""
import math

import numpy as np

F32 = np.float32
MIN_SIZE = 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


def cv_round(v: float) -> int:
    """cvRound: round half to even."""
    return int(round(v))


def level_plan(H, W, pyr_scale, levels):
    """[(k, scale_k, h_k, w_k, sigma_k, ksize_k)] for k = levels' .. 0, with levels' cut by the 32-pixel rule."""
    scale = 1.0
    k = 0
    while k < levels:
        scale *= pyr_scale
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    plan = []
    for lv in range(k, -1, -1):
        s = 1.0
        for _ in range(lv):
            s *= pyr_scale
        sigma = (1.0 / s - 1) * 0.5
        ks = max(cv_round(sigma * 5) | 1, 3)
        plan.append((lv, s, cv_round(H * s), cv_round(W * s), sigma, ks))
    return plan


def gaussian_taps(n, sigma):
    """getGaussianKernel(n, sigma, CV_32F): float32 taps, normalised in float64 (the fixed [1/4, 1/2, 1/4] for n = 3, sigma <= 0)."""
    if sigma <= 0:
        assert n == 3
        return np.array([0.25, 0.5, 0.25], dtype=F32)
    scale2 = -0.5 / (sigma * sigma)
    cf = np.empty(n, dtype=F32)
    total = 0.0
    for i in range(n):
        x = i - (n - 1) * 0.5
        cf[i] = F32(math.exp(scale2 * x * x))
        total += float(cf[i])
    total = 1.0 / total
    for i in range(n):
        cf[i] = F32(float(cf[i]) * total)
    return cf


def reflect101(i, n):
    """BORDER_REFLECT_101 index map (any number of reflections)."""
    i = np.asarray(i, dtype=np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        lo, hi = i < 0, i >= n
        if not (lo.any() or hi.any()):
            return i
        i = np.where(lo, -i, np.where(hi, 2 * n - 2 - i, i))


def gaussian_blur(img, ksize, sigma):
    """GaussianBlur(img, (ksize, ksize), sigma, sigma), BORDER_REFLECT_101, float32: the row pass, then the column pass, each
    ``k0 * s[0] + sum_j k_j * (s[-j] + s[+j])`` in float32."""
    k = gaussian_taps(ksize, sigma)
    r = ksize // 2
    H, W = img.shape
    c = np.arange(W)
    t = img[:, c] * k[r]
    for j in range(1, r + 1):
        t = t + k[r + j] * (img[:, reflect101(c - j, W)] + img[:, reflect101(c + j, W)])
    rr = np.arange(H)
    out = t[rr] * k[r]
    for j in range(1, r + 1):
        out = out + k[r + j] * (t[reflect101(rr - j, H)] + t[reflect101(rr + j, H)])
    return out.astype(F32)


def _linear_coords(src, dst):
    """INTER_LINEAR source index / index + 1 / weight of the second tap for each destination index."""
    scale = 1.0 / (dst / src)
    f = np.array([F32((d + 0.5) * scale - 0.5) for d in range(dst)], dtype=F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    lo = s < 0
    f[lo], s[lo] = 0, 0
    hi = s >= src - 1
    f[hi], s[hi] = 0, src - 1
    return s, np.minimum(s + 1, src - 1), f


def resize_linear(src, h, w):
    """cv2.resize(src, (w, h), interpolation=INTER_LINEAR) for float32 [H, W] or [H, W, C]: the horizontal pass, then the vertical
    one, ``a * s0 + b * s1`` in float32."""
    H, W = src.shape[:2]
    if (H, W) == (h, w):
        return src.copy()
    sx0, sx1, fx = _linear_coords(W, w)
    sy0, sy1, fy = _linear_coords(H, h)
    if src.ndim == 3:
        fx = fx[:, None]
    t = src[:, sx0] * (F32(1) - fx) + src[:, sx1] * fx
    fy = fy[:, None] if src.ndim == 2 else fy[:, None, None]
    return (t[sy0] * (F32(1) - fy) + t[sy1] * fy).astype(F32)


def poly_exp_setup(n, sigma):
    """FarnebackPrepareGaussian: taps g, xg, xxg over x = -n..n (float32) and ig11, ig03, ig33, ig55 of the inverse Gram matrix."""
    if sigma < np.finfo(np.float32).eps:
        sigma = n * 0.3
    xs = range(-n, n + 1)
    g = np.array([F32(math.exp(-x * x / (2 * sigma * sigma))) for x in xs], dtype=F32)
    s = 1.0 / sum(float(v) for v in g)
    g = np.array([F32(float(v) * s) for v in g], dtype=F32)
    xg = np.array([F32(x) * g[x + n] for x in xs], dtype=F32)
    xxg = np.array([F32(x * x) * g[x + n] for x in xs], dtype=F32)
    G00 = G11 = G33 = G55 = 0.0
    for y in xs:
        for x in xs:
            gg = g[y + n] * g[x + n]
            G00 += float(gg)
            G11 += float(gg * F32(x) * F32(x))
            G33 += float(gg * F32(x) * F32(x) * F32(x) * F32(x))
            G55 += float(gg * F32(x) * F32(x) * F32(y) * F32(y))
    # the {1, x^2, y^2} block [[a, b, b], [b, c, d], [b, d, c]] inverted in closed form
    a, b, c, d = G00, G11, G33, G55
    q = a * (c + d) - 2 * b * b
    ig03 = -b / q
    ig33 = (a * c - b * b) / ((c - d) * q)
    return g, xg, xxg, 1.0 / G11, ig03, ig33, 1.0 / G55


def poly_exp(img, n, sigma):
    """FarnebackPolyExp -> R [5, H, W] float32: (b_row, b_col, A_rowrow, A_colcol, 2 A_rowcol) of the local fit
    c + b^T p + p^T A p, p = (row, col).  Vertical pass in float32 with replicated rows, horizontal pass in float64 with replicated
    columns."""
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_exp_setup(n, sigma)
    H, W = img.shape
    rows = np.arange(H)
    v0 = img * g[n]
    v1 = np.zeros_like(img)
    v2 = np.zeros_like(img)
    for k in range(1, n + 1):
        up = img[np.maximum(rows - k, 0)]
        dn = img[np.minimum(rows + k, H - 1)]
        p = up + dn
        v0 = v0 + g[n + k] * p
        v1 = v1 + xg[n + k] * (dn - up)
        v2 = v2 + xxg[n + k] * p
    cols = np.arange(W)
    D = np.float64
    b1 = (v0 * g[n]).astype(D)
    b3 = (v1 * g[n]).astype(D)
    b5 = (v2 * g[n]).astype(D)
    b2 = np.zeros((H, W))
    b4 = np.zeros((H, W))
    b6 = np.zeros((H, W))
    for k in range(1, n + 1):
        lf, rt = np.maximum(cols - k, 0), np.minimum(cols + k, W - 1)
        tg = (v0[:, rt] + v0[:, lf]).astype(D)
        b1 = b1 + tg * D(g[n + k])
        b4 = b4 + tg * D(xxg[n + k])
        b2 = b2 + ((v0[:, rt] - v0[:, lf]) * xg[n + k]).astype(D)
        b3 = b3 + ((v1[:, rt] + v1[:, lf]) * g[n + k]).astype(D)
        b6 = b6 + ((v1[:, rt] - v1[:, lf]) * xg[n + k]).astype(D)
        b5 = b5 + ((v2[:, rt] + v2[:, lf]) * g[n + k]).astype(D)
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55]).astype(F32)


def _border_scale(i, n):
    s = np.ones(i.shape, dtype=F32)
    for d in range(5):
        s = np.where(i == d, s * F32(BORDER[d]), s) if d < n else s
    return s


def update_matrices(R0, R1, flow):
    """FarnebackUpdateMatrices at every pixel -> M [5, H, W] float32 (G11, G12, G22, h1, h2).  flow: [2, H, W] (dx, dy)."""
    _, H, W = R0.shape
    dx, dy = flow[0], flow[1]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx = xx.astype(F32) + dx
    fy = yy.astype(F32) + dy
    x1 = np.floor(fx).astype(np.int64)
    y1 = np.floor(fy).astype(np.int64)
    fx = fx - x1.astype(F32)
    fy = fy - y1.astype(F32)
    inside = (x1 >= 0) & (x1 < W - 1) & (y1 >= 0) & (y1 < H - 1)
    xc, yc = np.clip(x1, 0, max(W - 2, 0)), np.clip(y1, 0, max(H - 2, 0))
    xc1, yc1 = np.minimum(xc + 1, W - 1), np.minimum(yc + 1, H - 1)
    one = F32(1)
    a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    r = [a00 * R1[c][yc, xc] + a01 * R1[c][yc, xc1] + a10 * R1[c][yc1, xc] + a11 * R1[c][yc1, xc1] for c in range(5)]
    half, quarter = F32(0.5), F32(0.25)
    r2 = np.where(inside, r[0], F32(0))
    r3 = np.where(inside, r[1], F32(0))
    r4 = np.where(inside, (R0[2] + r[2]) * half, R0[2])
    r5 = np.where(inside, (R0[3] + r[3]) * half, R0[3])
    r6 = np.where(inside, (R0[4] + r[4]) * quarter, R0[4] * half)
    r2 = (R0[0] - r2) * half
    r3 = (R0[1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    xr = np.arange(W)
    yr = np.arange(H)
    sx0, sx1 = _border_scale(xr, W)[None, :], _border_scale(W - 1 - xr, W)[None, :]
    sy0, sy1 = _border_scale(yr, H)[:, None], _border_scale(H - 1 - yr, H)[:, None]
    scale = ((sx0 * sx1) * sy0) * sy1
    near = ((xr < 5) | (xr >= W - 5))[None, :] | ((yr < 5) | (yr >= H - 5))[:, None]
    r2, r3, r4, r5, r6 = (np.where(near, v * scale, v) for v in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3]).astype(F32)


def box_sum(M, m):
    """(2m+1)^2 replicate-border window sums of M [C, H, W] in float64."""
    P = np.pad(M.astype(np.float64), ((0, 0), (m, m), (m, m)), mode="edge")
    c = np.cumsum(np.pad(P, ((0, 0), (1, 0), (0, 0))), axis=1)
    v = c[:, 2 * m + 1:] - c[:, :-2 * m - 1]
    c = np.cumsum(np.pad(v, ((0, 0), (0, 0), (1, 0))), axis=2)
    return c[:, :, 2 * m + 1:] - c[:, :, :-2 * m - 1]


def solve_flow(M, winsize):
    """FarnebackUpdateFlow_Blur's solve: the window sums scaled by 1 / winsize^2, then the regularised 2 x 2 system."""
    S = box_sum(M, winsize // 2) * (1.0 / (winsize * winsize))
    g11, g12, g22, h1, h2 = S
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet]).astype(F32)


def level_image(frame, scale, h, w, sigma, ksize):
    """The level-k image: the full-resolution frame in float32, blurred, resized to (h, w)."""
    img = np.asarray(frame).astype(F32)
    return resize_linear(gaussian_blur(img, ksize, sigma), h, w)


def calc_optical_flow_farneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags=0):
    """cv2.calcOpticalFlowFarneback(prev, next, flow, ...) for flags 0 -> [H, W, 2] float32 (dx, dy); ``flow`` is ignored."""
    assert flags == 0
    prev, next = np.asarray(prev), np.asarray(next)
    H, W = prev.shape
    prev_flow = None
    for lv, s, h, w, sigma, ks in level_plan(H, W, pyr_scale, levels):
        if prev_flow is None:
            fl = np.zeros((2, h, w), dtype=F32)
        else:
            fl = (resize_linear(prev_flow.transpose(1, 2, 0), h, w) * F32(1.0 / pyr_scale)).transpose(2, 0, 1).astype(F32)
        R0 = poly_exp(level_image(prev, s, h, w, sigma, ks), poly_n, poly_sigma)
        R1 = poly_exp(level_image(next, s, h, w, sigma, ks), poly_n, poly_sigma)
        M = update_matrices(R0, R1, fl)
        for it in range(iterations):
            fl = solve_flow(M, winsize)
            if it < iterations - 1:
                M = update_matrices(R0, R1, fl)
        prev_flow = fl
    return np.ascontiguousarray(prev_flow.transpose(1, 2, 0))
