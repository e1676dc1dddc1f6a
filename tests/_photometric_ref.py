"""The photometric functions restated in torch on the CPU, in the project's own words: what csrc/photometric.hip has to compute.
tests/test_photometric.py pins these to the reference's own outputs (tests/golden/golden_photometric.npz) exactly, in float64 and
in float32, and compares the kernels against them on the GPU, where the reference itself does not exist.
"""
import math

import torch
import torch.nn.functional as F


def taps(window_size=11, dtype=torch.float32):
    """The SSIM window: a Gaussian of sigma 1.5, float32 from the start, normalised, its outer product, cast last."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)], dtype=torch.float32)
    g = (g / g.sum())[:, None]
    return (g @ g.t()).to(dtype)


def base_grid(h, w):
    """The normalised pixel grid in torch's default dtype (float32): an integer tensor divided by a Python float."""
    rows, cols = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return rows / ((h - 1) / 2.0) - 1, cols / ((w - 1) / 2.0) - 1


def normalised(flow):
    """flow [2, H, W] -> the normalised sample coordinates (rows, columns) in the flow's dtype."""
    h, w = flow.shape[-2:]
    gr, gc = base_grid(h, w)
    return gr - flow[0] / ((h - 1) / 2.0), gc - flow[1] / ((w - 1) / 2.0)


def sample(image, nr, nc):
    """image [H, W] bilinearly at the normalised coordinates, corners aligned, zeros outside."""
    grid = torch.stack([nc, nr], dim=-1)[None]
    return F.grid_sample(image[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]


def warp_forward(image, flow):
    """image [H, W] (any dtype; taken in the flow's), flow [2, H, W] -> the image sampled at x - flow."""
    return sample(image.to(flow.dtype), *normalised(flow))


def warp_shift(image, shift):
    """image [H, W] float64, shift [2]: a 0-dim shift does not promote the float32 grid, so the coordinates are float32 whatever the
    shift's dtype; then the image is sampled in float64."""
    h, w = image.shape
    gr, gc = base_grid(h, w)
    nr, nc = gr - shift[0] / ((h - 1) / 2.0), gc - shift[1] / ((w - 1) / 2.0)
    return sample(image, nr.double(), nc.double())


def positions(flow):
    """The sample positions in pixels (rows, columns), as grid_sample un-normalises them."""
    h, w = flow.shape[-2:]
    nr, nc = normalised(flow)
    return (nr + 1) * ((h - 1) / 2.0), (nc + 1) * ((w - 1) / 2.0)


def counted(flow, roi=None, mask=None):
    """bool [H, W]: inside the roi, mask non-zero, flow finite, all four bilinear taps inside the image."""
    h, w = flow.shape[-2:]
    pr, pc = positions(flow)
    r0, c0 = torch.floor(pr), torch.floor(pc)
    ok = (r0 >= 0) & (r0 + 1 <= h - 1) & (c0 >= 0) & (c0 + 1 <= w - 1) & torch.isfinite(flow[0]) & torch.isfinite(flow[1])
    if roi is not None:
        inside = torch.zeros(h, w, dtype=torch.bool)
        inside[roi[0]:roi[1], roi[2]:roi[3]] = True
        ok = ok & inside
    if mask is not None:
        ok = ok & (torch.as_tensor(mask) != 0)
    return ok


def near_boundary(flow, tol):
    """bool [H, W]: a sample position within ``tol`` of an integer, where float32 and float64 may pick different taps."""
    pr, pc = positions(flow)
    near = (torch.abs(pr - torch.round(pr)) < tol) | (torch.abs(pc - torch.round(pc)) < tol)
    return near & torch.isfinite(pr) & torch.isfinite(pc)


def ssim_map(img1, img2, window_size=11):
    """[B, C, H, W] pairs -> the SSIM map: five windowed moments under the taps, zero padding."""
    c = img1.shape[1]
    k = taps(window_size, img1.dtype)[None, None].expand(c, 1, window_size, window_size).contiguous()
    conv = lambda x: F.conv2d(x, k, padding=window_size // 2, groups=c)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu12
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))


def ssim_reference_mean(img1, img2, window_size=11, size_average=True):
    """The mean as the reference takes it: in the input dtype."""
    m = ssim_map(img1, img2, window_size)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def exact_mean(values):
    """The float64 mean as the package defines it: the exact sum of the values (``math.fsum``) rounded once, then divided."""
    v = values.double().reshape(-1).tolist()
    return math.fsum(v) / len(v)


def ssim_mean(img1, img2, window_size=11, size_average=True):
    """The exact float64 mean of the map (or of each item's part of it), cast to the input dtype."""
    m = ssim_map(img1, img2, window_size)
    if size_average:
        return torch.tensor(exact_mean(m), dtype=torch.float64).to(img1.dtype)
    return torch.tensor([exact_mean(x) for x in m], dtype=torch.float64).to(img1.dtype)


COLUMNS = ("L1", "RMSE", "SSIM", "L1_0", "RMSE_0", "SSIM_0", "n_points")


def score(frame1, frame2, flow, roi=None, mask=None, window_size=11, drop=None):
    """One item: frame1, frame2 [H, W], flow [2, H, W] (its dtype is the compute type) -> float64 [7].  Per-pixel values in the
    compute type, exact float64 means over the counted pixels (minus ``drop``, a bool map, when given)."""
    T = flow.dtype
    f1, f2 = frame1.to(T), frame2.to(T)
    ok = counted(flow, roi, mask)
    if drop is not None:
        ok = ok & ~drop
    n = int(ok.sum())
    out = torch.full((7,), float("nan"), dtype=torch.float64)
    out[6] = n
    if n == 0:
        return out
    for k, w in ((0, warp_forward(f1, flow)), (3, f1)):
        d = (w - f2)[ok]
        q = ssim_map(w[None, None], f2[None, None], window_size)[0, 0][ok]
        out[k] = exact_mean(torch.abs(d))
        out[k + 1] = math.sqrt(exact_mean(d * d))
        out[k + 2] = exact_mean(q)
    return out
