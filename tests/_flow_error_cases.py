"""Inputs of the flow-error fixture (tests/golden/golden_flow_error.npz), regenerated from seeds, and an independent numpy
restatement of the reference's metrics (src/utils/flow_utils.py:706-823) that the tests hold the fixture and the GPU against.

Only the seeds, a few edits and the reference's outputs are stored; ``case_inputs(name)`` rebuilds a case's
(flow_gt, flow_pred, event_mask, time_scale) exactly as tests/golden/make_golden_flow_error.py handed them to the reference.
"""
import numpy as np

KEYS = ("EPE", "1PE", "2PE", "3PE", "5PE", "10PE", "20PE", "AE")
THRESHOLDS = (1.0, 2.0, 3.0, 5.0, 10.0, 20.0)
ROI_HW = (720, 640)              # the ROI of the shipped YAML
SENSOR_HW = (720, 1280)
ROI = {"xmin": 0, "xmax": 720, "ymin": 320, "ymax": 960}
SMALL_HW = (96, 128)

# name -> variant ("numpy" = calculate_flow_error_numpy on float64, "tensor32" = calculate_flow_error_tensor on float32 CPU torch)
CASES = {
    "roi_nomask": "numpy",        # float64 720 x 640, no mask
    "roi_mask4": "numpy",         # ... a [1, 1, H, W] mask
    "roi_mask3": "numpy",         # ... a [1, H, W] mask
    "batch3": "numpy",            # B = 3 with per-item masks
    "gt_special": "numpy",        # GT with zero components, inf and NaN
    "pred_nan_out": "numpy",      # NaN in pred outside the mask
    "pred_eq_gt": "numpy",        # pred == gt: the reference's AE is NaN
    "thresholds": "numpy",        # differences exactly at 1, 2, 3, 5, 10, 20 px
    "tensor_f32_ts": "tensor32",  # float32 torch with time_scale
    "solver_roi": "numpy",        # 720 x 1280 flows, ROI view, mask from events (create_eventmask)
}


def _flows(rs, shape, spread=3.0):
    gt = rs.uniform(-8.0, 8.0, shape)
    pred = gt + rs.normal(0.0, spread, shape)
    return gt, pred


def solver_events(n=100_000, seed=11):
    """[n, 4] float64 events (x = row, y = column, t, p) over the 720 x 1280 sensor, fractional coordinates."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(0, SENSOR_HW[0] - 1, n)
    y = rs.uniform(0, SENSOR_HW[1] - 1, n)
    t = np.sort(rs.uniform(0, 0.01, n))
    p = rs.randint(0, 2, n).astype(np.float64)
    return np.stack([x, y, t, p], axis=1)


def case_inputs(name, golden=None):
    """(flow_gt, flow_pred, event_mask | None, time_scale | None) of a case.  ``solver_roi`` returns the [1, 2, 720, 640] ROI views
    of 720 x 1280 flows and, as mask, the reference's event mask unpacked from ``golden`` (None without it)."""
    H, W = ROI_HW
    if name in ("roi_nomask", "roi_mask4", "roi_mask3"):
        rs = np.random.RandomState(1)
        gt, pred = _flows(rs, (1, 2, H, W))
        m = rs.uniform(size=(H, W)) < 0.3
        mask = None if name == "roi_nomask" else (m[None, None] if name == "roi_mask4" else m[None])
        return gt, pred, mask, None
    if name == "batch3":
        rs = np.random.RandomState(2)
        gt, pred = _flows(rs, (3, 2) + SMALL_HW, spread=6.0)
        mask = rs.uniform(size=(3, 1) + SMALL_HW) < np.array([0.2, 0.5, 0.9])[:, None, None, None]
        return gt, pred, mask, None
    if name in ("gt_special", "pred_nan_out"):
        rs = np.random.RandomState(3 if name == "gt_special" else 4)
        gt, pred = _flows(rs, (1, 2) + SMALL_HW)
        mask = rs.uniform(size=(1, 1) + SMALL_HW) < 0.6
        if name == "gt_special":
            gt[0, 0, :10, :] = 0.0            # zero u: excluded
            gt[0, 1, 20:25, 5:50] = 0.0       # zero v: excluded
            gt[0, 0, 40, 7] = np.inf          # inf: excluded, but inf * 0 makes the sums NaN
            gt[0, 1, 50, 9] = np.nan          # NaN
            return gt, pred, mask, None
        out = np.argwhere(~mask[0, 0])[:5]
        pred[0, 0, out[:, 0], out[:, 1]] = np.nan
        return gt, pred, mask, None
    if name == "pred_eq_gt":
        rs = np.random.RandomState(5)
        gt, _ = _flows(rs, (1, 2, H, W))
        return gt, gt.copy(), None, None
    if name == "thresholds":
        rs = np.random.RandomState(6)
        gt, pred = _flows(rs, (1, 2) + SMALL_HW, spread=4.0)
        gt = np.round(gt * 4) / 4
        gt[gt == 0] = 0.5
        for k, (du, dv) in enumerate([(1, 0), (0, -2), (3, 0), (0, 5), (6, 8), (12, 16)]):
            for j in range(3):
                r, c = 7 * k + j, 11 * j + k
                gt[0, :, r, c] = (7.0, 9.0)
                pred[0, 0, r, c] = 7.0 - du
                pred[0, 1, r, c] = 9.0 - dv
        return gt, pred, None, None
    if name == "tensor_f32_ts":
        rs = np.random.RandomState(7)
        gt, pred = _flows(rs, (2, 2) + SMALL_HW, spread=2.0)
        mask = rs.uniform(size=(2, 1) + SMALL_HW) < 0.5
        return gt.astype(np.float32), pred.astype(np.float32), mask, np.array([0.5, 2.0], dtype=np.float32)
    if name == "solver_roi":
        rs = np.random.RandomState(8)
        gt_full, pred_full = _flows(rs, (2,) + SENSOR_HW)
        sl = (slice(None), slice(ROI["xmin"], ROI["xmax"]), slice(ROI["ymin"], ROI["ymax"]))
        mask = None
        if golden is not None:
            mask = np.unpackbits(golden["solver_roi_mask_bits"])[:H * W].reshape(1, H, W).astype(bool)
        return gt_full[sl][None], pred_full[sl][None], mask, None
    raise KeyError(name)


def restated_flow_error(gt, pred, mask=None, time_scale=None):
    """Per-item [B, 9] table (EPE, 1PE, 2PE, 3PE, 5PE, 10PE, 20PE, AE, count) and the batch means, in float64.  float32 flows are
    masked, scaled and differenced in float32 (the reference's elementwise ops) and normed in float64, as the GPU kernel does."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    B, _, H, W = gt.shape
    valid = ~np.isinf(gt[:, 0]) & ~np.isinf(gt[:, 1])   # (NaN passes this and fails the next test)
    with np.errstate(invalid="ignore"):
        valid &= (np.abs(gt[:, 0]) > 0) & (np.abs(gt[:, 1]) > 0)
    if mask is not None:
        m = np.asarray(mask)
        m = m.reshape((1,) * (4 - m.ndim) + m.shape)
        valid &= np.broadcast_to(m != 0, (B, 1, H, W))[:, 0]
    w = valid.astype(gt.dtype)
    table = np.zeros((B, 9))
    with np.errstate(invalid="ignore", over="ignore"):
        gu, gv, pu, pv = gt[:, 0] * w, gt[:, 1] * w, pred[:, 0] * w, pred[:, 1] * w
        if time_scale is not None:
            ts = np.asarray(time_scale, dtype=gt.dtype).reshape(B, 1, 1)
            gu, gv, pu, pv = gu * ts, gv * ts, pu * ts, pv * ts
        dx, dy = (gu - pu).astype(np.float64), (gv - pv).astype(np.float64)
        e = np.sqrt(dx * dx + dy * dy)
        u, v, ug, vg = (a.astype(np.float64) for a in (pu, pv, gu, gv))
        cos = (1.0 + u * ug + v * vg) / (np.sqrt(1.0 + u * u + v * v) * np.sqrt(1.0 + ug * ug + vg * vg))
        ae = np.arccos(cos)
    for b in range(B):
        cnt = int(valid[b].sum())
        n = cnt + 1e-5
        table[b, 0] = e[b].sum() / n
        for j, k in enumerate(THRESHOLDS):
            table[b, 1 + j] = np.count_nonzero(e[b] > k) / n
        table[b, 7] = ae[b].sum() / n
        table[b, 8] = cnt
    return table, table.mean(axis=0)
