"""Plain torch float64 restatement of the reference's generative patch-pyramid solver (src/solver/patch_eklt_pyramid2.py on
patch_eklt_dependent.py, patch_eklt.py and generative_max_likelihood.py), op for op, with autograd and torch.optim.Adam.

It is the CPU checker of the HIP solver (tests/test_gpu_gml.py) and is itself pinned to the reference by
tests/golden/golden_gml.npz (tests/test_gml.py).  ``device`` may be a GPU: tools/bench_gml.py times it there as the eager
baseline.  OpenCV's Sobel / GaussianBlur / resize are restated in numpy (BORDER_REFLECT_101, the float64 kernel size
round(8 sigma + 1) | 1); scipy's gaussian_filter is scipy's own.
"""
import numpy as np
import scipy.ndimage
import torch
import torch.nn.functional as F

PATCHES = (64, 32, 16, 8)   # prepare_pyramidal_patch(shape, 64, 8): scales 1..4, slide = patch
FINEST_SCALE = 5


# ------------------------------------------------------------------ OpenCV restated (numpy, float64)
def cv_sobel(f):
    """(cv2.Sobel(f, CV_64F, 0, 1, ksize=3), cv2.Sobel(f, CV_64F, 1, 0, ksize=3)): d/d row, d/d column, reflect-101."""
    p = np.pad(np.asarray(f, dtype=np.float64), 1, mode="reflect")
    sm_c = p[:, :-2] + 2.0 * p[:, 1:-1] + p[:, 2:]          # [1 2 1] along columns
    sm_r = p[:-2, :] + 2.0 * p[1:-1, :] + p[2:, :]          # [1 2 1] along rows
    gx = sm_c[2:, :] - sm_c[:-2, :]
    gy = sm_r[:, 2:] - sm_r[:, :-2]
    return gx, gy


def cv_gaussian_taps(sigma):
    n = int(round(float(sigma) * 8 + 1)) | 1
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    t = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return t * (1.0 / t.sum())


def _conv_reflect101(img, taps, axis):
    r = len(taps) // 2
    L = img.shape[axis]
    idx = np.arange(-r, L + r)
    period = 2 * (L - 1)
    idx = np.abs(np.mod(idx, period))
    idx = np.where(idx >= L, period - idx, idx)
    src = np.take(img, idx, axis=axis)
    out = np.zeros_like(img)
    for k, w in enumerate(taps):
        out = out + w * np.take(src, np.arange(k, k + L), axis=axis)
    return out


def cv_gaussian_blur(img, sigma):
    """cv2.GaussianBlur(img, ksize=None, sigmaX=sigma) for float64: rows, then columns, BORDER_REFLECT_101."""
    taps = cv_gaussian_taps(sigma)
    return _conv_reflect101(_conv_reflect101(np.asarray(img, dtype=np.float64), taps, 1), taps, 0)


# ------------------------------------------------------------------ measurement (calculate_iwe_cache, _make_measured_increment)
def polarity_image(events, shape):
    """The numpy polarity IWE with sigma 0 (src/event_image_converter.py:355-363): bilinear votes of p > 0 and of p <= 0."""
    from oracle import ebos_oracle as O
    return O.polarity_numpy(np.asarray(events, dtype=np.float64), tuple(shape))


def prepare(frame, pol, gml, roi):
    """-> dict of numpy float64: gx, gy (of the model image), hist (cache_histogram), we (cache_weights or None), winv, mask."""
    f = np.asarray(frame, dtype=np.float64)
    if gml.get("use_log_intensity"):
        f = np.log(f + 1).astype(float)
    gx, gy = cv_sobel(f)
    hist = pol[0] + pol[1] if gml.get("no_polarity") else pol[0] - pol[1]
    we = cv_gaussian_blur(np.abs(hist), gml["weight_sigma"]) if gml.get("weight_loss_by_event_hist") else None
    cache = cv_gaussian_blur(hist, gml["iwe_sigma"]) if gml.get("iwe_sigma") else hist.copy()
    if gml.get("weight_loss_by_inverse_event_hist"):
        wi = scipy.ndimage.gaussian_filter(np.abs(hist), 10)
        wi = np.clip(wi, 0, wi.mean() + wi.std() / 2.)
        wi /= wi.max()
        wi = 1.0 - 0.95 * wi
    else:
        wi = np.ones_like(hist)
    H, W = hist.shape
    mask = np.zeros((H, W))
    mask[roi[0]:roi[1], roi[2]:roi[3]] = 1
    return {"gx": gx, "gy": gy, "hist": cache, "we": we, "winv": wi, "mask": mask}


def measured(st):
    """_make_measured_increment of pyramid2: divides cache_histogram IN PLACE when there are no weights (once per scale)."""
    if st["we"] is not None:
        m = st["we"] * st["hist"]
    else:
        m = st["hist"]
    m /= np.linalg.norm(m)
    return m


# ------------------------------------------------------------------ patch grid and model (torch)
def grid_shape(H, W, p):
    return len(np.arange(0, H - p + p, p)), len(np.arange(0, W - p + p, p))


def upsample(grid, p, H, W):
    """interpolate_dense_flow_from_patch_tensor at patch = slide = p: [c, gh, gw] -> [c, H, W]."""
    c, gh, gw = grid.shape
    pad = int(p / 2 // p) + 1
    g = F.pad(grid.reshape(1, c, gh, gw), (pad, pad, pad, pad), mode="replicate")[0]
    size = [g.shape[1] * p, g.shape[2] * p]
    dense = F.interpolate(g[None], size=size, mode="bilinear", align_corners=False)[0]
    cx, cy = dense.shape[1] // 2, dense.shape[2] // 2
    h1, w1 = cx - H // 2, cy - W // 2
    return dense[..., h1:h1 + H, w1:w1 + W]


_GX = [[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]]
_GY = [[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]


def sobel_patch(pot):
    """poisson_to_flow: SobelTorch(in_channels=1, ksize=3, replicate padding)(pot[None, None]) / 8 -> [2, gh, gw]."""
    k = torch.tensor([[_GX], [_GY]], dtype=pot.dtype, device=pot.device)   # [2, 1, 3, 3]
    x = F.pad(pot.reshape(1, 1, *pot.shape[-2:]), (1, 1, 1, 1), mode="replicate")
    return (F.conv2d(x, k) / 8.)[0]


def warp_forward(im, flow):
    """frame_utils.warp_image_forward on tensors: the base grid in the default (float32) dtype, float64 flow subtracted."""
    h, w = im.shape
    coord_x, coord_y = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    coord_x = coord_x[None, None] / ((h - 1) / 2.0) - 1
    coord_y = coord_y[None, None] / ((w - 1) / 2.0) - 1
    warp_x = coord_x.to(flow.device) - flow[None][:, [0]] / ((h - 1) / 2.0)
    warp_y = coord_y.to(flow.device) - flow[None][:, [1]] / ((w - 1) / 2.0)
    grid = torch.cat([warp_y, warp_x], dim=1).permute((0, 2, 3, 1))
    return F.grid_sample(im[None, None], grid, mode="bilinear", align_corners=True)[0, 0]


class Model(object):
    """The objective of one window at one scale (``_objective_scipy`` of pyramid2)."""

    def __init__(self, st, gml, cost, p, q, device="cpu"):
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).double().to(device)
        self.gx, self.gy, self.winv, self.mask = t(st["gx"]), t(st["gy"]), t(st["winv"]), t(st["mask"])
        self.we, self.q = t(st["we"]), t(q)
        self.H, self.W = st["gx"].shape
        self.gml, self.cost, self.p = gml, dict(cost), p

    def parts(self, x):
        """-> (loss, {term: value}) as torch scalars (HybridCost.calculate, terms in the configuration's order)."""
        H, W, p, M = self.H, self.W, self.p, self.mask
        Fd = upsample(sobel_patch(x[0]), p, H, W)
        gx, gy = self.gx.clone(), self.gy.clone()
        T = None
        if self.gml["optimize_warp"]:
            T = upsample(x[[-2, -1]], p, H, W)
            gx, gy = warp_forward(gx, T), warp_forward(gy, T)
        P = Fd[0] * gx + Fd[1] * gy
        if self.gml["no_polarity"]:
            P = torch.abs(P)
        if self.we is not None:
            P = P * (self.we * M)
        P = P / (torch.linalg.norm(P.clone()) + 0.0001)
        P = P * M
        Q = self.q * M
        loss, terms = 0.0, {}
        for name, wgt in self.cost.items():
            if name == "diff_norm":
                v = torch.linalg.norm(Q - P, ord=1)
            elif name == "image_gradient":
                fl = Fd * M
                v = torch.mean(torch.abs(torch.gradient(fl, dim=1)[0] * self.winv) + torch.abs(torch.gradient(fl, dim=2)[0] * self.winv))
            elif name == "flow_norm_pxy":
                v = torch.linalg.norm(T * M, dim=0).mean()
            else:
                raise NotImplementedError(name)
            terms[name] = v
            loss = loss + wgt * v
        return loss, terms

    def margin(self, x):
        """(largest - second largest) / largest column sum of |Q M - P|: how far the diff_norm subgradient is from a tie."""
        with torch.no_grad():
            H, W, p, M = self.H, self.W, self.p, self.mask
            Fd = upsample(sobel_patch(x[0]), p, H, W)
            gx, gy = self.gx, self.gy
            if self.gml["optimize_warp"]:
                T = upsample(x[[-2, -1]], p, H, W)
                gx, gy = warp_forward(gx, T), warp_forward(gy, T)
            P = Fd[0] * gx + Fd[1] * gy
            if self.gml["no_polarity"]:
                P = torch.abs(P)
            if self.we is not None:
                P = P * (self.we * M)
            P = P / (torch.linalg.norm(P) + 0.0001) * M
            cs = torch.abs(self.q * M - P).sum(0)
            top = torch.topk(cs, 2).values
            return float((top[0] - top[1]) / top[0])


def initial_potentials(n_dim, gh, gw):
    """x0 of the coarsest scale: np.concatenate([init() for _ in patches]).reshape(n_dim, gh, gw), init() = [u, 0, 0] with u
    from numpy's GLOBAL RandomState, after one discarded draw (a reshape, not a transpose: the draws land in every n_dim-th slot of all channels)."""
    np.random.random()   # run_estimation_per_scale first calls init() once for n_parameter_dim: that draw is discarded
    rows = []
    for _ in range(gh * gw):
        base = np.random.random() * 2. - 1
        rows.append(np.array([base, 0., 0.] if n_dim == 3 else [base], dtype=np.float64))
    return np.concatenate(rows).reshape((n_dim, gh, gw))


def resize_params(x, gh, gw):
    """torchvision resize(x_coarser, (gh, gw)), bilinear, up-sampling only."""
    return F.interpolate(x[None], size=[gh, gw], mode="bilinear", align_corners=False)[0]


def solve(frame, events, gml, cost, n_iter, roi, init_seed=None, device="cpu", want_margin=False, pol=None):
    """One ``estimate`` of the reference.  -> dict: history {loss, <term>...} (lists), params [x per scale], flow [2, H, W],
    margins (list, if want_margin)."""
    H, W = np.asarray(frame).shape
    if pol is None:
        pol = polarity_image(events, (H, W))
    st = prepare(frame, pol, gml, roi)
    if init_seed is not None:
        np.random.seed(init_seed)
    n_dim = 3 if gml["optimize_warp"] else 1
    hist = {"loss": []}
    hist.update({k: [] for k in cost})
    params, margins, x_prev = [], [], None
    for s, p in enumerate(PATCHES, start=1):
        gh, gw = grid_shape(H, W, p)
        if x_prev is None:
            x0 = torch.from_numpy(initial_potentials(n_dim, gh, gw)).double().to(device)
        else:
            x0 = resize_params(x_prev, gh, gw)
        x = x0.clone().requires_grad_()
        model = Model(st, gml, cost, p, measured(st), device)
        iters = n_iter // (FINEST_SCALE - s + 1)
        opt = torch.optim.Adam([x], lr=0.05)
        for _ in range(iters):
            opt.zero_grad()
            loss, terms = model.parts(x)
            if want_margin:
                margins.append(model.margin(x.detach()))
            hist["loss"].append(float(loss.detach()))
            for k, v in terms.items():
                hist[k].append(float(v.detach()))
            loss.backward()
            opt.step()
        x_prev = x.detach()
        params.append(x_prev.cpu().numpy().copy())
    with torch.no_grad():
        flow = upsample(sobel_patch(x_prev[0]), PATCHES[-1], H, W) * torch.from_numpy(st["mask"]).to(device)
    out = {"history": {k: np.array(v) for k, v in hist.items()}, "params": params, "flow": flow.cpu().numpy()}
    if want_margin:
        out["margins"] = np.array(margins)
    return out


def objective_and_grad(st, gml, cost, p, q, x, device="cpu"):
    """(loss, {term: value}, d loss / d x) by autograd, as floats / numpy."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().to(device).requires_grad_()
    loss, terms = Model(st, gml, cost, p, q, device).parts(xt)
    loss.backward()
    return float(loss.detach()), {k: float(v.detach()) for k, v in terms.items()}, xt.grad.cpu().numpy()


__all__ = ["PATCHES", "FINEST_SCALE", "cv_sobel", "cv_gaussian_blur", "cv_gaussian_taps", "prepare", "measured", "grid_shape",
           "upsample", "sobel_patch", "warp_forward", "Model", "initial_potentials", "resize_params", "solve",
           "objective_and_grad", "polarity_image"]
