"""numpy restatement of ``cv2.warpPerspective`` (INTER_LINEAR, BORDER_CONSTANT 0) for float64 single-channel images: the warp of
the model image's gradients in the reference's sampled EKLT solvers (src/solver/generative_max_likelihood.py:504-513), and the
arithmetic contract of csrc/eklt_sweep.hip.

It is tests/_warp_ref.py's classic path (coordinates per block origin, times 32, rounded half to even, 5 fraction bits) with the
float64 pixel type: the four tap weights are the FLOAT32 products of the bilinear table -- (1 - fy, fy) x (1 - fx, fx) of the 1/32
fractions -- and the sum ``((s00 w00 + s01 w01) + s10 w10) + s11 w11`` is taken in double.  A tap outside the source is 0; a pixel
whose four taps all lie outside is 0.  As _warp_ref.py, it is not checked against OpenCV, which is absent where this package is
developed.

``translation(p_x, p_y)`` is the reference's matrix: p_x moves rows, p_y columns.  ``shift_and_weights`` is what a translation
comes to for EVERY pixel when 32 p is not within rounding of a half-integer: one integer shift per axis and four weights.
"""
import numpy as np

from _warp_ref import INTER_BITS, INTER_TAB_SIZE, _sat16, coordinates, invert3x3


def translation(p_x, p_y):
    return np.array([[1, 0, p_y], [0, 1, p_x], [0, 0, 1]], dtype=np.float64)


def table_weights(fy, fx):
    """The float32 table entries of fractions (fy, fx) in 1/32 units, widened -> (w00, w01, w10, w11) float64 arrays."""
    step = np.float32(1.0 / INTER_TAB_SIZE)
    bx, by = np.asarray(fx).astype(np.float32) * step, np.asarray(fy).astype(np.float32) * step
    ax, ay = np.float32(1) - bx, np.float32(1) - by
    return tuple(np.asarray(w, dtype=np.float32).astype(np.float64) for w in (ay * ax, ay * bx, by * ax, by * bx))


def warp_perspective_f64(src, M, dsize):
    """src [Hs, Ws] float64; M 3 x 3; dsize (W, H) as in cv2 -> [H, W] float64."""
    src = np.asarray(src, dtype=np.float64)
    assert src.ndim == 2
    W, H = int(dsize[0]), int(dsize[1])
    Hs, Ws = src.shape
    X, Y = coordinates(invert3x3(M), (W, H), False)
    sx, sy = _sat16(X >> INTER_BITS), _sat16(Y >> INTER_BITS)
    fx, fy = X & (INTER_TAB_SIZE - 1), Y & (INTER_TAB_SIZE - 1)

    def tap(ty, tx):
        inside = (tx >= 0) & (tx < Ws) & (ty >= 0) & (ty < Hs)
        return np.where(inside, src[np.clip(ty, 0, Hs - 1), np.clip(tx, 0, Ws - 1)], 0.0), inside

    (s00, i00), (s01, i01), (s10, i10), (s11, i11) = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    w00, w01, w10, w11 = table_weights(fy, fx)
    out = ((s00 * w00 + s01 * w01) + s10 * w10) + s11 * w11
    return np.where(i00 | i01 | i10 | i11, out, 0.0)


def shift_and_weights(p_x, p_y):
    """-> (s_r, s_c, (w00, w01, w10, w11)): destination (r, c) reads source rows r + s_r, r + s_r + 1 and columns c + s_c,
    c + s_c + 1.  The coordinate of the image's first pixel, as the classic path rounds it."""
    Y = int(np.rint((0.0 - float(p_x)) * 32.0))
    X = int(np.rint((0.0 - float(p_y)) * 32.0))
    w = table_weights(Y & (INTER_TAB_SIZE - 1), X & (INTER_TAB_SIZE - 1))
    return Y >> INTER_BITS, X >> INTER_BITS, tuple(float(v) for v in w)


def half_integer_margin(p):
    """Distance of 32 p from the nearest half-integer: the 1/32 rounding is the same for every pixel while this exceeds the
    rounding of ``x - p`` (below 1e-9 for any image)."""
    v = 32.0 * np.asarray(p, dtype=np.float64)
    return np.abs(v - np.floor(v) - 0.5)
