"""A vectorised numpy restatement of the reference's event filters (src/utils/event_filters.py:46-128), exact for any window size:
the check for GPU runs far too large for the reference's per-event loops.  tests/test_event_filters.py pins it on the
reference's own outputs (tests/golden/golden_filters.npz)."""
import numpy as np


def baf_numpy(ev, shape, dt, ksize, num_support, m0=None):
    """continuous_background_activity_filter -> (kept events, final time map).  The map at pixel q when event i is looked at is
    m0[q] maxed with the times of q's events of index <= i: events grouped by (pixel, index), an inclusive prefix max per pixel
    run (exact, through integer ranks of the times), and for every neighbour offset a search for the last slot of the run
    with index <= i."""
    H, W = shape
    n = len(ev)
    m0 = np.zeros(shape) if m0 is None else np.asarray(m0, dtype=np.float64)
    x = np.trunc(ev[:, 0]).astype(np.int64)                    # int(x)
    y = np.trunc(ev[:, 1]).astype(np.int64)
    t = ev[:, 2].astype(np.float64)
    if n and (x.min() < 0 or x.max() >= H or y.min() < 0 or y.max() >= W):
        raise ValueError("event outside the sensor")
    key = x * W + y
    order = np.argsort(key, kind="stable")
    sk = key[order]
    uniq, rank = np.unique(t[order], return_inverse=True)
    m = len(uniq)
    pm = uniq[np.maximum.accumulate(sk * m + rank) % m]          # per-run inclusive prefix max of t
    combo = sk * n + order                                     # sorted, unique
    vals, npx = [], np.zeros(n, dtype=np.int64)
    for dr in range(-ksize, ksize + 1):
        for dc in range(-ksize, ksize + 1):
            qr, qc = x + dr, y + dc
            inside = (qr >= 0) & (qr < H) & (qc >= 0) & (qc < W)
            q = np.where(inside, qr * W + qc, 0)
            pos = np.searchsorted(combo, q * n + np.arange(n), side="right") - 1
            hit = (pos >= 0) & (sk[np.maximum(pos, 0)] == q)
            v = np.where(hit, np.maximum(m0.reshape(-1)[q], pm[np.maximum(pos, 0)]), m0.reshape(-1)[q])
            vals.append(np.where(inside, v, -np.inf))
            npx += inside
    vals = np.sort(np.stack(vals, 1), axis=1)
    if n and (npx < num_support + 1).any():
        raise IndexError("clipped neighbourhood")
    last = vals[:, -1 - num_support] if n else np.zeros(0)
    keep = t - last < dt
    mf = m0.copy().reshape(-1)
    if n:
        ends = np.r_[np.flatnonzero(np.diff(sk)), n - 1]
        mf[sk[ends]] = np.maximum(mf[sk[ends]], pm[ends])
    return ev[keep], mf.reshape(shape)


def hot_numpy(ev, shape, thresh):
    """hot_pixel_filter for integer coordinates: the sigma = 0 image is the per-pixel count."""
    H, W = shape
    key = np.trunc(ev[:, 0]).astype(np.int64) * W + np.trunc(ev[:, 1]).astype(np.int64)
    cnt = np.bincount(key, minlength=H * W)
    return ev[~(cnt[key] > thresh)]


def decode_window(g, name):
    """float64 [n, 4] window ``name`` of the stored fixture (tests/golden/make_golden_filters.py): pixel + fraction / 65536,
    t = microseconds / 1e6, p; rows with an explicit float64 x."""
    xy = g[f"win_{name}_xy"].astype(np.float64)
    if f"win_{name}_fxy" in g:
        xy = xy + g[f"win_{name}_fxy"] / 65536.0
    ev = np.empty((len(xy), 4), dtype=np.float64)
    ev[:, :2] = xy
    ev[:, 2] = g[f"win_{name}_t"] / 1e6
    ev[:, 3] = g[f"win_{name}_p"]
    if f"win_{name}_ovr_idx" in g:
        ev[g[f"win_{name}_ovr_idx"], 0] = g[f"win_{name}_ovr_x"]
    return ev


def load_golden_filters(path):
    """tests/golden/golden_filters.npz expanded to arrays per case: ``<case>_events`` / ``_kept`` / ``_map`` / ``_m0`` /
    ``_params`` and ``seq_<c>_w<k>_in`` / ``_out`` / ``_map`` / ``seq_<c>_config``."""
    g = dict(np.load(path, allow_pickle=False))
    H, W = (int(v) for v in g["shape"])
    wins = {k[4:-3]: decode_window(g, k[4:-3]) for k in g if k.startswith("win_") and k.endswith("_xy")}

    def final_map(key, base, f32):
        m = base.copy().reshape(-1)
        if f"{key}_map_as" in g:
            key = str(g[f"{key}_map_as"])
        names = [str(v) for v in g[f"{key}_wins"]]
        for w, r in zip(g[f"{key}_map_w"], g[f"{key}_map_row"]):
            e = wins[names[w]][r]
            if f32:
                e = e.astype(np.float32)
            m[int(e[0]) * W + int(e[1])] = np.float64(e[2])
        return m.reshape(H, W)

    out = {}
    for key in [k[:-len("_params")] for k in g if k.endswith("_params")]:
        f32 = bool(g[f"{key}_f32"])
        ev = wins[str(g[f"{key}_win"])]
        ev = ev.astype(np.float32) if f32 else ev
        out[f"{key}_events"], out[f"{key}_kept"], out[f"{key}_params"] = ev, ev[g[f"{key}_kept_idx"]], g[f"{key}_params"]
        if f"{key}_m0_idx" in g:
            m0 = np.zeros(H * W)
            m0[g[f"{key}_m0_idx"]] = g[f"{key}_m0_val"]
            out[f"{key}_m0"] = m0.reshape(H, W)
            out[f"{key}_map"] = final_map(key, out[f"{key}_m0"], f32)
    for c in (0, 1):
        out[f"seq_{c}_config"] = g[f"seq_{c}_config"]
        for k in range(3):
            w = wins[f"seq{k}"]
            out[f"seq_{c}_w{k}_in"], out[f"seq_{c}_w{k}_out"] = w, w[g[f"seq_{c}_w{k}_kept_idx"]]
            out[f"seq_{c}_w{k}_map"] = final_map(f"seq_{c}_w{k}", np.zeros((H, W)), False)
    return out
