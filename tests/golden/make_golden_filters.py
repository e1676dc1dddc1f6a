#!/usr/bin/env python3
"""Generate tests/golden/golden_filters.npz by running the REFERENCE's event filters (src/utils/event_filters.py) on seeded
synthetic windows.  Runs only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_filters.py

Storage (kept small; tests/_filter_ref.py:load_golden_filters expands it to per-case arrays ``<case>_events`` input,
``<case>_kept`` reference output, ``<case>_map`` final BAF time map, ``<case>_m0`` start map, ``<case>_params`` =
(dt, ksize, num_support_event) for BAF or (thresh,) for HOT; ``seq_<c>_w<k>_in`` / ``_out`` / ``_map``):
  win_<w>_xy / _t / _p     every input window ONCE as sensor-style columns: pixel int16 [n, 2], t int32 microseconds, p uint8;
  win_<w>_fxy              (fractional windows) + fraction / 65536 per coordinate; win_<w>_ovr_idx / _ovr_x: rows whose x is
                           given as a float64 instead (719.9999999-style values).  The float64 window the reference ran on is
                           decode(storage) -- the generator builds every input that way -- and ``<case>_f32`` = 1 marks a case
                           whose input is that window cast to float32
  <case>_kept_idx          rows of the input the reference kept, in order (its output is exactly those rows)
  <case>_map_w / _map_row  the final map as the events whose times it holds: window number (into ``<case>_wins``) and row, one per
                           pixel that differs from the start map; ``<case>_map_as`` instead names a case with the same events
  <case>_m0_idx / _val     the non-zero pixels of the start map
The generator asserts that every decoded output equals the reference's array exactly.

Cases:
  baf_*     continuous_background_activity_filter (:46-97) at 346 x 260 on sparse uniform noise + moving edges, times partly out of
            order, k in {0, 1, 2}, s in {0, 1, 2, 3}; a float32 window; a non-zero start map; events on borders and corners;
            fractional coordinates
  hot_*     hot_pixel_filter (:100-128): integer windows with hot pixels, some of them exactly at the threshold (kept: `>`),
            and a fractional window whose bilinear image keeps every pixel further than 1e-9 from the threshold
  seq_<c>_* EventFilter (:154-224) with CROP -> BAF -> HOT over three windows (``win_seq<k>``, the same for both c),
            BAF_continuous_update c in {0, 1}: ``seq_<c>_w<k>_kept_idx`` / ``_map_idx`` / ``_map_val`` (the filter's time
            map after window k, against zeros); window 2 falls under the 10-event rule after CROP
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from _filter_ref import decode_window, load_golden_filters  # noqa: E402

H, W = 260, 346
OUT = os.path.join(HERE, "golden_filters.npz")


def noise_and_edges(rs, n_noise, n_edge, t_span=0.05, h=H, w=W, shuffle_frac=0.1):
    """Uniform background noise + two edges sweeping across the sensor (correlated events), time-sorted, then a fraction of the
    events swapped with a neighbour a few places on (times out of order)."""
    xn, yn = rs.randint(0, h, n_noise), rs.randint(0, w, n_noise)
    tn = rs.uniform(0, t_span, n_noise)
    te = np.sort(rs.uniform(0, t_span, n_edge))
    half = n_edge // 2
    col = (20 + (w - 40) * te / t_span + rs.normal(0, 0.7, n_edge)).astype(int)
    row = rs.randint(0, h, n_edge)
    row[half:] = (20 + (h - 40) * te[half:] / t_span + rs.normal(0, 0.7, n_edge - half)).astype(int)
    col[half:] = rs.randint(0, w, n_edge - half)
    xe, ye = np.clip(row, 0, h - 1), np.clip(col, 0, w - 1)
    ev = np.concatenate([np.stack([xn, yn, tn, rs.randint(0, 2, n_noise)], 1), np.stack([xe, ye, te, rs.randint(0, 2, n_edge)], 1)])
    ev = ev[np.argsort(ev[:, 2], kind="stable")].astype(np.float64)
    k = rs.choice(len(ev) - 5, int(shuffle_frac * len(ev)), replace=False)
    j = k + rs.randint(1, 5, len(k))
    ev[[k, j]] = ev[[j, k]]
    return ev


def main():
    import_reference()
    from src.utils import event_filters as F

    rs = np.random.RandomState(1234)
    out = {"shape": np.array([H, W])}

    def put_window(name, ev, frac=False, ovr=None):
        """Store the window as columns; returns the float64 window those columns decode to (what the reference is given)."""
        out[f"win_{name}_xy"] = np.floor(ev[:, :2]).astype(np.int16)
        out[f"win_{name}_t"] = np.rint(ev[:, 2] * 1e6).astype(np.int32)
        out[f"win_{name}_p"] = ev[:, 3].astype(np.uint8)
        if frac:
            out[f"win_{name}_fxy"] = np.floor((ev[:, :2] - np.floor(ev[:, :2])) * 65536).astype(np.uint16)
        if ovr is not None:
            out[f"win_{name}_ovr_idx"], out[f"win_{name}_ovr_x"] = ovr[0].astype(np.int32), ovr[1].astype(np.float64)
        return decode_window(out, name)

    def rows_of(ev, kept):
        """Indices of the input rows the reference kept: its output is exactly those rows, in order."""
        kept = np.asarray(kept).reshape(-1, 4)
        idx, j = [], 0
        for i in range(len(ev)):
            if j < len(kept) and np.array_equal(ev[i], kept[j]):
                idx.append(i)
                j += 1
        idx = np.array(idx, dtype=np.int32)
        assert j == len(kept) and np.array_equal(ev[idx], kept.astype(ev.dtype)), "kept events are not rows of the input in order"
        return idx

    def put_map(key, m, base, wins, f32=False):
        """The final map as the events whose times it holds (BAF sets a pixel to the time of one of its events)."""
        d = np.flatnonzero(m.reshape(-1) != base.reshape(-1))
        want, src = set(d.tolist()), {}
        for w, name in enumerate(wins):
            ev = windows[name].astype(np.float32) if f32 else windows[name]
            pix = np.trunc(ev[:, 0]).astype(np.int64) * W + np.trunc(ev[:, 1]).astype(np.int64)
            hit = np.flatnonzero(np.isin(pix, d) & (m.reshape(-1)[pix] == ev[:, 2].astype(np.float64)))
            for r in hit:
                src.setdefault(int(pix[r]), (w, int(r)))
        assert set(src) == want, "a map value is no event's time"
        mw, mr = np.array([src[q][0] for q in d], dtype=np.uint8), np.array([src[q][1] for q in d], dtype=np.int32)
        for other, (ow, orow, owins) in maps.items():   # (the final map does not depend on dt, ksize or num_support_event)
            if owins == wins and np.array_equal(ow, mw) and np.array_equal(orow, mr):
                out[f"{key}_map_as"] = np.array(other)
                return
        maps[key] = (mw, mr, list(wins))
        out[f"{key}_map_w"], out[f"{key}_map_row"], out[f"{key}_wins"] = mw, mr, np.array(wins)

    maps = {}

    def put_m0(key, m0):
        d = np.flatnonzero(m0.reshape(-1)).astype(np.int32)
        out[f"{key}_m0_idx"], out[f"{key}_m0_val"] = d, m0.reshape(-1)[d]

    windows = {}

    def baf(name, win, dt, k, s, m0=None, f32=False, shape=(H, W)):
        ev = windows[win].astype(np.float32) if f32 else windows[win]
        m0 = np.zeros(shape) if m0 is None else m0
        kept, m = F.continuous_background_activity_filter(ev, shape, dt, k, s, time_map=m0.copy())
        out[f"{name}_win"], out[f"{name}_f32"] = np.array(win), np.array(int(f32))
        out[f"{name}_kept_idx"] = rows_of(ev, kept)
        put_m0(name, m0)
        put_map(name, m, m0, [win], f32=f32)
        out[f"{name}_params"] = np.array([dt, k, s], dtype=np.float64)
        expect[name] = (np.asarray(kept).reshape(-1, 4), m)
        print(f"{name}: {len(ev)} events, BAF kept {len(out[name + '_kept_idx'])} ({100.0 * len(out[name + '_kept_idx']) / len(ev):.1f} %)")

    expect = {}

    base = windows["base"] = put_window("base", noise_and_edges(rs, 1500, 6500))
    for k, s in ((1, 1), (1, 0), (2, 3), (0, 0), (1, 2), (2, 1)):
        baf(f"baf_k{k}s{s}", "base", 0.006, k, s)
    baf("baf_f32", "base", 0.006, 1, 1, f32=True)
    m0 = np.where(rs.uniform(size=(H, W)) < 0.02, np.rint(rs.uniform(-0.01, 0.02, (H, W)) * 1e6) / 1e6, 0.0)
    windows["m0"] = put_window("m0", noise_and_edges(rs, 1000, 2000))
    baf("baf_m0", "m0", 0.004, 1, 1, m0=m0)
    # borders and corners: every event on the outer two rows / columns, the four corners many times
    nb = 2500
    side = rs.randint(0, 4, nb)
    pos = rs.randint(0, max(H, W), nb)
    off = rs.randint(0, 2, nb)
    bx = np.where(side == 0, off, np.where(side == 1, H - 1 - off, pos % H))
    by = np.where(side == 2, off, np.where(side == 3, W - 1 - off, pos % W))
    corners = np.array([[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]])[rs.randint(0, 4, 400)]
    bxy = np.concatenate([np.stack([bx, by], 1), corners])
    windows["border"] = put_window("border", np.concatenate([bxy, rs.uniform(0, 0.05, (len(bxy), 1)), rs.randint(0, 2, (len(bxy), 1))], 1))
    baf("baf_border", "border", 0.003, 2, 3)
    baf("baf_border_k1", "border", 0.003, 1, 1)
    # fractional coordinates (pixel = int(x) of the float64 value, 719.9999999-style values included)
    frac = base[:3000].copy()
    frac[:, :2] += rs.randint(0, 65536, (len(frac), 2)) / 65536.0
    ovr = np.arange(0, len(frac), 97)
    windows["frac"] = put_window("frac", frac, frac=True, ovr=(ovr, np.floor(frac[ovr, 0]) + 0.9999999))
    baf("baf_frac", "frac", 0.006, 1, 1)

    def hot(name, win, thresh, f32=False):
        ev = windows[win].astype(np.float32) if f32 else windows[win]
        kept = F.hot_pixel_filter(ev, (H, W), thresh)
        out[f"{name}_win"], out[f"{name}_f32"] = np.array(win), np.array(int(f32))
        out[f"{name}_kept_idx"] = rows_of(ev, kept)
        out[f"{name}_params"] = np.array([thresh], dtype=np.float64)
        expect[name] = (np.asarray(kept).reshape(-1, 4), None)
        print(f"{name}: {len(ev)} events, HOT kept {len(out[name + '_kept_idx'])}")

    # hot pixels: 12 pixels far above the threshold, 6 exactly at it (kept), 6 one above it (dropped)
    thresh = 10
    hp = rs.randint(0, [H, W], (24, 2))
    counts = np.r_[rs.randint(40, 400, 12), np.full(6, thresh), np.full(6, thresh + 1)]
    hx = np.repeat(hp, counts, axis=0)
    hev = np.concatenate([hx, rs.uniform(0, 0.05, (len(hx), 1)), rs.randint(0, 2, (len(hx), 1))], 1)
    ev = np.concatenate([base[:4000], hev])
    ev = windows["hot"] = put_window("hot", ev[rs.permutation(len(ev))])
    hot("hot_int", "hot", thresh)
    hot("hot_int_f32", "hot", thresh, f32=True)
    # fractional: bilinear image with no pixel within 1e-9 of the threshold (accumulation order cannot flip a decision)
    fev = ev[:5000].copy()
    fev[:, :2] = np.minimum(fev[:, :2] + rs.randint(3277, 62259, (len(fev), 2)) / 65536.0, [H - 1.5, W - 1.5])
    fev = windows["hotfrac"] = put_window("hotfrac", fev, frac=True)
    fth = 4.5
    from src.event_image_converter import EventImageConverter

    iwe = EventImageConverter((H, W)).create_iwe(fev, sigma=0)
    assert np.abs(iwe - fth).min() > 1e-9, "a fractional pixel value lies within 1e-9 of the threshold"
    assert (iwe > fth).sum() > 0
    hot("hot_frac", "hotfrac", fth)

    # EventFilter: CROP -> BAF -> HOT over three windows
    rsw = np.random.RandomState(77)
    for k in range(3):
        if k < 2:
            w = noise_and_edges(rsw, 1000, 2000, shuffle_frac=0.05)
            w[:, 2] += 0.05 * k
            w = np.concatenate([w, np.repeat([[100 + k, 200, 0.05 * k + 0.01, 1]], 30, 0)])   # a hot pixel
        else:
            w = np.concatenate([rsw.randint(0, 5, (40, 2)), 0.1 + rsw.uniform(0, 0.05, (40, 1)), np.ones((40, 1))], 1)  # 6 after CROP
            w[:6, :2] = [50, 60]
        windows[f"seq{k}"] = put_window(f"seq{k}", w)
    for cont in (0, 1):
        cfg = {"filters": ["BAF", "HOT"], "parameters": {"BAF_dt": 0.004, "BAF_ksize": 1, "BAF_num_support_event": 1,
                                                         "BAF_continuous_update": bool(cont), "HOT_thresh": 10,
                                                         "xmin": 10, "xmax": 250, "ymin": 20, "ymax": 330}}
        ef = F.EventFilter((H, W), cfg)
        for k in range(3):
            w = windows[f"seq{k}"]
            res = ef.process(w)
            tm = np.zeros((H, W)) if ef.time_map is None else ef.time_map.copy()
            out[f"seq_{cont}_w{k}_kept_idx"] = rows_of(w, res)
            put_map(f"seq_{cont}_w{k}", tm, np.zeros((H, W)), [f"seq{j}" for j in range(k + 1)])
            expect[f"seq_{cont}_w{k}"] = (np.asarray(res).reshape(-1, 4), tm)
            print(f"seq cont={cont} window {k}: {len(w)} -> {len(out[f'seq_{cont}_w{k}_kept_idx'])}")
        out[f"seq_{cont}_config"] = np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)

    np.savez_compressed(OUT, **out)
    # the stored form gives back exactly what the reference computed
    g = load_golden_filters(OUT)
    for name, (kept, m) in expect.items():
        if name.startswith("seq_"):
            assert np.array_equal(g[name + "_out"], kept) and np.array_equal(g[name + "_map"], m), name
        else:
            assert np.array_equal(g[name + "_kept"], kept) and g[name + "_kept"].dtype == kept.dtype, name
            if m is not None:
                assert np.array_equal(g[name + "_map"], m), name
    print(OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
