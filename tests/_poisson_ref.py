"""An independent numpy restatement of the reference's Poisson integration (src/utils/stat_utils.py:142-199) and of the
visualizer's uint8 picture (src/visualizer.py:432-433), as dense DST matrices in float64: the form csrc/poisson.hip computes.

    P = S_h^T ((S_h F S_w^T) / D) S_w

S_N is scipy's orthonormal DST-II matrix, its inverse (ortho DST-III) is S_N^T, D holds the 5-point Laplacian's eigenvalues.
"""
import numpy as np


def dst_matrix(N):
    """Orthonormal DST-II: S[k, n] = c_k 2 sin(pi m / (2N)), m = (k+1)(2n+1) mod 4N (exact integers), c_k = sqrt(1 / (2N)) but
    c_{N-1} = sqrt(1 / (4N))."""
    k = np.arange(N, dtype=np.int64)[:, None]
    n = np.arange(N, dtype=np.int64)[None, :]
    m = ((k + 1) * (2 * n + 1)) % (4 * N)
    c = np.full((N, 1), np.sqrt(1.0 / (2 * N)))
    c[N - 1] = np.sqrt(1.0 / (4 * N))
    return c * (2.0 * np.sin(np.pi * m / (2 * N)))


def divergence(grady, gradx, boundarysrc):
    """F (h x w, float64): the differences in the input dtype, summed into float64, minus the boundary's stencil in its dtype."""
    H, W = boundarysrc.shape
    f = np.zeros((H, W))
    f[:-1, 1:] += gradx[:-1, 1:] - gradx[:-1, :-1]
    f[1:, :-1] += grady[1:, :-1] - grady[:-1, :-1]
    b = boundarysrc.copy()
    b[1:-1, 1:-1] = 0
    stencil = -4 * b[1:-1, 1:-1] + b[1:-1, 2:] + b[1:-1, 0:-2] + b[2:, 1:-1] + b[0:-2, 1:-1]
    return f[1:-1, 1:-1] - stencil


def eigenvalues(H, W):
    i = np.arange(1, H - 1)[:, None]
    j = np.arange(1, W - 1)[None, :]
    return (2 * np.cos(np.pi * j / W) - 2) + (2 * np.cos(np.pi * i / H) - 2)


def restated_poisson(grady, gradx, boundarysrc):
    """poisson_reconstruct(grady, gradx, boundarysrc): boundarysrc with its interior replaced by P, in boundarysrc's dtype."""
    H, W = boundarysrc.shape
    F = divergence(grady, gradx, boundarysrc)
    Sh, Sw = dst_matrix(H - 2), dst_matrix(W - 2)
    G = (Sh @ F @ Sw.T) / eigenvalues(H, W)
    P = Sh.T @ G @ Sw
    out = boundarysrc.copy()
    out[1:-1, 1:-1] = 0
    out[1:-1, 1:-1] = P
    return out


def standardized(P):
    """standardize_image_center(P) before the cast, in P's dtype (src/utils/frame_utils.py:39-53)."""
    return (P - 0) / np.abs(P).max() * (255 - 128) + 128


def restated_image(P):
    """The visualizer's uint8 picture of P; an all-zero P gives 128 (the package's documented difference)."""
    if not np.abs(P).max() > 0:
        return np.full(P.shape, 128, dtype=np.uint8)
    return standardized(P).astype(np.uint8)
