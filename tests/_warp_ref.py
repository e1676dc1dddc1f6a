"""numpy restatement of ``cv2.warpPerspective`` (INTER_LINEAR / INTER_NEAREST, BORDER_CONSTANT, optional WARP_INVERSE_MAP) for
uint8 and float32 single-channel frames: the arithmetic contract of csrc/frame_warp.hip.

What this is and is not.  It restates OpenCV's classic algorithm -- the fixed-point path of OpenCV 4.5 - 4.10 -- and is not checked
against OpenCV, which is absent where this package is developed (the same standing as tests/_farneback_ref.py).  OpenCV >= 4.11's
newer linear path may differ in the last grey level.

The algorithm, step by step:

* the matrix is inverted in float64 unless WARP_INVERSE_MAP: the closed-form cofactor inverse times ONE reciprocal of the determinant;
* the destination is walked in blocks ``bh = min(16, H)``, ``bw = min(1024 // bh, W)``, ``bh = min(1024 // bw, H)``; for a pixel
  (x, y) of the block whose first column is x0: ``X0 = M0 x0 + M1 y + M2`` (likewise Y0, W0), then ``X = (X0 + M0 x1) s`` with
  x1 = x - x0 and ``s = 32 / (W0 + M6 x1)`` (0 where that sum is 0; ``1 / ...`` for INTER_NEAREST), every product and sum rounded on
  its own (no fused multiply-add), clamped to the int32 range with C's fmin / fmax (a NaN becomes INT_MAX) and rounded half to even;
* INTER_LINEAR: the tap is ``X >> 5`` saturated to int16 and the fraction ``X & 31`` per axis; uint8 frames take the four 15-bit
  weights of the 32 x 32 table (``interp_table``) and give ``(sum S w + 16384) >> 15``; float32 frames take the float products of
  the same fractions, accumulated left to right;
* BORDER_CONSTANT: a tap outside the source takes the border value; a pixel whose four taps all lie outside IS the border value;
* INTER_NEAREST: the rounded quotient is the tap.

A pixel's value never depends on ``roi``: the rectangle only selects which pixels are returned.
"""
import numpy as np

INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16
INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS
COEF_BITS = 15
COEF_SCALE = 1 << COEF_BITS
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def invert3x3(M: np.ndarray) -> np.ndarray:
    """The closed-form inverse: cofactors times one reciprocal of the determinant, float64, unfused.  Singular -> ValueError."""
    m = np.asarray(M, dtype=np.float64).reshape(3, 3)
    det = m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) \
        + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])
    if det == 0 or not np.isfinite(det):
        raise ValueError("singular matrix")
    d = 1.0 / det
    t = np.empty(9)
    t[0] = (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d
    t[1] = (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d
    t[2] = (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d
    t[3] = (m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d
    t[4] = (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d
    t[5] = (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d
    t[6] = (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d
    t[7] = (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d
    t[8] = (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d
    return t.reshape(3, 3)


def block_width(H: int, W: int) -> int:
    bh = min(16, H)
    bw = min(1024 // bh, W)
    return bw


def interp_table() -> np.ndarray:
    """[32 (fy), 32 (fx), 2, 2] int32: the float32 products (1 - fy, fy) x (1 - fx, fx) of the 1/32 fractions, times 32768, rounded
    and saturated to int16; where the four do not sum to 32768 (only fy = fx = 0, whose single weight saturates at 32767) the
    largest takes the difference."""
    f = np.arange(INTER_TAB_SIZE, dtype=np.float32) * np.float32(1.0 / INTER_TAB_SIZE)
    lin = np.stack([np.float32(1) - f, f], axis=1)                                     # [32, 2]
    v = lin[:, None, :, None] * lin[None, :, None, :]                                  # [fy, fx, ky, kx] float32
    tab = np.clip(np.rint(v * np.float32(COEF_SCALE)), -32768, 32767).astype(np.int32)
    flat = tab.reshape(-1, 4)
    diff = flat.sum(axis=1) - COEF_SCALE
    for i in np.nonzero(diff)[0]:
        flat[i, np.argmax(flat[i])] -= diff[i]
    return flat.reshape(INTER_TAB_SIZE, INTER_TAB_SIZE, 2, 2)


def border_as(dtype, border_value):
    if np.dtype(dtype) == np.uint8:
        return np.uint8(min(255, max(0, int(np.rint(border_value)))))
    return np.float32(border_value)


def coordinates(Minv: np.ndarray, dsize, nearest: bool, rows=None, cols=None):
    """Integer source coordinates (X, Y) int64 [h, w] of destination rows ``rows`` and columns ``cols`` (default: all): scaled by 32
    for INTER_LINEAR, whole pixels for INTER_NEAREST."""
    W, H = int(dsize[0]), int(dsize[1])
    m = np.asarray(Minv, dtype=np.float64).reshape(9)
    bw = block_width(H, W)
    x = np.arange(W, dtype=np.int64) if cols is None else np.asarray(cols, dtype=np.int64)
    y = np.arange(H, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    x0 = ((x // bw) * bw).astype(np.float64)[None, :]
    x1 = (x % bw).astype(np.float64)[None, :]
    yy = y.astype(np.float64)[:, None]
    X0 = (m[0] * x0 + m[1] * yy) + m[2]
    Y0 = (m[3] * x0 + m[4] * yy) + m[5]
    W0 = (m[6] * x0 + m[7] * yy) + m[8]
    Wd = W0 + m[6] * x1
    num = 1.0 if nearest else float(INTER_TAB_SIZE)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.where(Wd != 0, num / np.where(Wd != 0, Wd, 1.0), 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        # fmin / fmax drop a NaN (inf * 0 where 32 / W overflows) as C's do: such a coordinate becomes INT_MAX, outside every source
        fX = np.fmax(float(INT_MIN), np.fmin(float(INT_MAX), (X0 + m[0] * x1) * s))
        fY = np.fmax(float(INT_MIN), np.fmin(float(INT_MAX), (Y0 + m[3] * x1) * s))
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)


def _sat16(v):
    return np.clip(v, -32768, 32767)


def warp_perspective(src, M, dsize, flags=INTER_LINEAR, border_value=0, roi=None):
    """src [Hs, Ws] uint8 | float32; M 3 x 3; dsize (W, H) as in cv2; roi (xmin, xmax, ymin, ymax) = destination rows
    [xmin, xmax) and columns [ymin, ymax) to return (the reference's common_params convention) -> [h, w] of src's dtype."""
    src = np.asarray(src)
    assert src.ndim == 2 and src.dtype in (np.uint8, np.float32)
    interp = flags & ~WARP_INVERSE_MAP
    assert interp in (INTER_NEAREST, INTER_LINEAR)
    W, H = int(dsize[0]), int(dsize[1])
    Minv = np.asarray(M, dtype=np.float64).reshape(3, 3) if flags & WARP_INVERSE_MAP else invert3x3(M)
    xmin, xmax, ymin, ymax = (0, H, 0, W) if roi is None else (int(v) for v in roi)
    assert 0 <= xmin < xmax <= H and 0 <= ymin < ymax <= W
    rows, cols = np.arange(xmin, xmax), np.arange(ymin, ymax)
    Hs, Ws = src.shape
    cval = border_as(src.dtype, border_value)
    X, Y = coordinates(Minv, (W, H), interp == INTER_NEAREST, rows, cols)

    def tap(sy, sx):
        inside = (sx >= 0) & (sx < Ws) & (sy >= 0) & (sy < Hs)
        v = src[np.clip(sy, 0, Hs - 1), np.clip(sx, 0, Ws - 1)]
        return np.where(inside, v, cval).astype(src.dtype), inside

    if interp == INTER_NEAREST:
        return tap(_sat16(Y), _sat16(X))[0]
    sx, sy = _sat16(X >> INTER_BITS), _sat16(Y >> INTER_BITS)
    fx, fy = X & (INTER_TAB_SIZE - 1), Y & (INTER_TAB_SIZE - 1)
    (s00, i00), (s01, i01), (s10, i10), (s11, i11) = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    none_inside = ~(i00 | i01 | i10 | i11)
    if src.dtype == np.uint8:
        w = interp_table()[fy, fx]                                                     # [h, w, 2, 2]
        acc = s00.astype(np.int64) * w[..., 0, 0] + s01.astype(np.int64) * w[..., 0, 1] + s10.astype(np.int64) * w[..., 1, 0] \
            + s11.astype(np.int64) * w[..., 1, 1]
        out = np.clip((acc + (1 << (COEF_BITS - 1))) >> COEF_BITS, 0, 255).astype(np.uint8)
    else:
        step = np.float32(1.0 / INTER_TAB_SIZE)
        bx, by = fx.astype(np.float32) * step, fy.astype(np.float32) * step
        ax, ay = np.float32(1) - bx, np.float32(1) - by
        out = ((s00 * (ay * ax) + s01 * (ay * bx)) + s10 * (by * ax)) + s11 * (by * bx)
        assert out.dtype == np.float32
    return np.where(none_inside, cval, out).astype(src.dtype)


def warp_perspective_batch(srcs, M, dsize, flags=INTER_LINEAR, border_value=0, roi=None):
    """srcs [B, Hs, Ws]; M [3, 3] (shared) or [B, 3, 3]."""
    M = np.asarray(M, dtype=np.float64)
    return np.stack([warp_perspective(s, M if M.ndim == 2 else M[b], dsize, flags, border_value, roi) for b, s in enumerate(srcs)])
