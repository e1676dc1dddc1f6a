"""Plain torch float64 restatement of the reference's single-scale generative solver (src/solver/patch_eklt_dependent.py on
patch_eklt.py and generative_max_likelihood.py), op for op, with autograd and torch.optim.Adam.

It is the CPU checker of the HIP solver (tests/test_gpu_gml_dep.py) and is itself pinned to the reference by
tests/golden/golden_gml_dep.npz (tests/test_gml_dep.py).  ``device`` may be a GPU: tools/bench_gml.py times it there as the eager
baseline.  The measurement (Sobel of the model image, blurred histogram, weights) is tests/_gml_ref.py's ``prepare``.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _gml_ref as R


def axis(L, p, s):
    """prepare_patch along one axis -> (centres, grid length, pad cells k, centre-crop offset h1)."""
    centres = np.arange(0, L - p + s, s) + p / 2
    g = len(centres)
    k = int(p / 2 // s) + 1
    return centres, g, k, (g + 2 * k) * s // 2 - L // 2


def grid_shape(H, W, p, s):
    return axis(H, p, s)[1], axis(W, p, s)[1]


def upsample(grid, p, s, H, W):
    """interpolate_dense_flow_from_patch_tensor: [c, gh, gw] -> [c, H, W] (replicate pad k, bilinear to (g + 2k) s, centre crop)."""
    c, gh, gw = grid.shape
    k = int(p / 2 // s) + 1
    g = F.pad(grid.reshape(1, c, gh, gw), (k, k, k, k), mode="replicate")[0]
    dense = F.interpolate(g[None], size=[g.shape[1] * s, g.shape[2] * s], mode="bilinear", align_corners=False)[0]
    cx, cy = dense.shape[1] // 2, dense.shape[2] // 2
    h1, w1 = cx - H // 2, cy - W // 2
    return dense[..., h1:h1 + H, w1:w1 + W]


def select(events, H, W, p, s, roi, thresholding, thres):
    """estimate_indices: the patches whose centre is in the ROI (inclusive) and, when thresholding, whose event box
    [int(c - ceil(p / 2)), int(c + floor(p / 2))) holds more than `thres` events."""
    cx, gh, _, _ = axis(H, p, s)
    cy, gw, _, _ = axis(W, p, s)
    xmin, xmax, ymin, ymax = roi
    ev = np.asarray(events, dtype=np.float64)
    out = []
    for i in range(gh):
        if cx[i] < xmin or xmax < cx[i]:
            continue
        x0, x1 = int(cx[i] - np.ceil(p / 2)), int(cx[i] + np.floor(p / 2))
        rows = (x0 <= ev[:, 0]) & (ev[:, 0] < x1) if thresholding else None
        for j in range(gw):
            if cy[j] < ymin or ymax < cy[j]:
                continue
            if thresholding:
                y0, y1 = int(cy[j] - np.ceil(p / 2)), int(cy[j] + np.floor(p / 2))
                n = int(np.count_nonzero(rows & (y0 <= ev[:, 1]) & (ev[:, 1] < y1)))
                if not n > thres:
                    continue
            out.append(i * gw + j)
    return np.array(out, dtype=np.int64)


def n_dim(gml):
    if gml.get("poisson_model"):
        return 3 if gml["optimize_warp"] else 1
    return 4 if gml["optimize_warp"] else 2


class Model(object):
    """The objective of one window (``_objective_scipy`` with the dependent's ``_make_prediction_torch``) on the sparse parameter
    vector of the selected patches, laid out as ``reshape(-1, n_dim).T``."""

    def __init__(self, st, gml, cost, p, s, roi, idx, device="cpu"):
        xmin, xmax, ymin, ymax = roi
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[xmin:xmax, ymin:ymax])).double().to(device)
        self.gx, self.gy, self.winv, self.we = t(st["gx"]), t(st["gy"]), t(st["winv"]), t(st["we"])
        m = st["hist"][xmin:xmax, ymin:ymax]
        if st["we"] is not None:
            m = st["we"][xmin:xmax, ymin:ymax] * m
        else:
            m = m.copy()
        m /= np.linalg.norm(m)
        self.q = torch.from_numpy(np.ascontiguousarray(m)).double().to(device)
        self.H, self.W = st["gx"].shape
        self.gh, self.gw = grid_shape(self.H, self.W, p, s)
        self.gml, self.cost, self.p, self.s, self.roi = gml, dict(cost), p, s, roi
        self.idx = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(device)
        self.nd = n_dim(gml)
        self.device = device

    def _scatter(self, rows):
        out = torch.zeros((len(rows), self.gh * self.gw), dtype=torch.float64, device=self.device)
        for c, v in enumerate(rows):
            out[c, self.idx] += v
        return out.reshape(len(rows), self.gh, self.gw)

    def flow_grid(self, x):
        P = x.reshape(-1, self.nd).T
        if self.gml.get("poisson_model"):
            pot = torch.zeros((self.nd, self.gh * self.gw), dtype=torch.float64, device=self.device)
            pot[:, self.idx] = P[0]
            return R.sobel_patch(pot.reshape(self.nd, self.gh, self.gw)[0])
        return self._scatter([P[0], P[1]])

    def warp_grid(self, x):
        P = x.reshape(-1, self.nd).T
        return self._scatter([P[-2], P[-1]])

    def dense_flow(self, x):
        return upsample(self.flow_grid(x), self.p, self.s, self.H, self.W)

    def parts(self, x):
        xmin, xmax, ymin, ymax = self.roi
        Fd = self.dense_flow(x)[:, xmin:xmax, ymin:ymax]
        gx, gy = self.gx.clone(), self.gy.clone()
        T = None
        if self.gml["optimize_warp"]:
            T = upsample(self.warp_grid(x), self.p, self.s, self.H, self.W)[:, xmin:xmax, ymin:ymax]
            gx, gy = R.warp_forward(gx, T), R.warp_forward(gy, T)
        P = Fd[0] * gx + Fd[1] * gy
        if self.gml["no_polarity"]:
            P = torch.abs(P)
        if self.we is not None:
            P = P * self.we
        P = P / (torch.linalg.norm(P.clone()) + 0.0001)
        loss, terms = 0.0, {}
        for name, wgt in self.cost.items():
            if name == "diff_norm":
                v = torch.linalg.norm(self.q - P, ord=1)
            elif name == "image_gradient":
                v = torch.mean(torch.abs(torch.gradient(Fd, dim=1)[0] * self.winv) + torch.abs(torch.gradient(Fd, dim=2)[0] * self.winv))
            elif name == "flow_norm_pxy":
                v = torch.linalg.norm(T, dim=0).mean()
            else:
                raise NotImplementedError(name)
            terms[name] = v
            loss = loss + wgt * v
        return loss, terms

    def to_grid(self, x):
        """The sparse vector as the [n_dim, gh, gw] grid (0 on unselected patches)."""
        P = torch.as_tensor(x).reshape(-1, self.nd).T
        return self._scatter(list(P)).cpu().numpy()

    def from_grid(self, grid):
        g = torch.as_tensor(np.asarray(grid)).reshape(self.nd, -1)[:, self.idx.cpu()]
        return g.T.reshape(-1).to(self.device)


def initial_vector(gml, n_sel):
    """x0 of ``estimate``: Poisson model -- one discarded draw, then [2 r - 1, 0, 0] (or [2 r - 1]) per selected patch from numpy's
    global RandomState; velocity model -- zeros."""
    nd = n_dim(gml)
    if not gml.get("poisson_model"):
        return np.zeros(nd * n_sel)
    np.random.random()
    rows = []
    for _ in range(n_sel):
        base = np.random.random() * 2. - 1
        rows.append(np.array([base, 0., 0.] if nd == 3 else [base], dtype=np.float64))
    return np.concatenate(rows)


def solve(frame, events, gml, cost, n_iter, roi, p, s, thresholding=False, thres=0, init_seed=None, device="cpu", pol=None):
    """One ``estimate`` of the reference.  -> dict: history {loss, <term>...}, indices, params [n_dim, gh, gw], flow [2, H, W]."""
    H, W = np.asarray(frame).shape
    if pol is None:
        pol = R.polarity_image(events, (H, W))
    st = R.prepare(frame, pol, gml, roi)
    idx = select(events, H, W, p, s, roi, thresholding, thres)
    if init_seed is not None:
        np.random.seed(init_seed)
    model = Model(st, gml, cost, p, s, roi, idx, device)
    x = torch.from_numpy(initial_vector(gml, len(idx))).double().to(device).requires_grad_()
    hist = {"loss": []}
    hist.update({k: [] for k in cost})
    opt = torch.optim.Adam([x], lr=0.05)
    for _ in range(n_iter):
        opt.zero_grad()
        loss, terms = model.parts(x)
        hist["loss"].append(float(loss.detach()))
        for k, v in terms.items():
            hist[k].append(float(v.detach()))
        loss.backward()
        opt.step()
    with torch.no_grad():
        flow = model.dense_flow(x.detach())
    return {"history": {k: np.array(v) for k, v in hist.items()}, "indices": idx, "params": model.to_grid(x.detach()),
            "flow": flow.cpu().numpy()}


def objective_and_grad(st, gml, cost, p, s, roi, idx, grid, device="cpu"):
    """(loss, {term: value}, d loss / d x as a [n_dim, gh, gw] grid) by autograd at the parameter grid `grid` (its selected
    cells)."""
    model = Model(st, gml, cost, p, s, roi, idx, device)
    x = model.from_grid(grid).clone().requires_grad_()
    loss, terms = model.parts(x)
    loss.backward()
    return float(loss.detach()), {k: float(v.detach()) for k, v in terms.items()}, model.to_grid(x.grad)


__all__ = ["axis", "grid_shape", "upsample", "select", "n_dim", "Model", "initial_vector", "solve", "objective_and_grad"]
