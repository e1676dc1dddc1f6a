#!/usr/bin/env python3
"""Generate tests/golden/golden_warp_voxel.npz: the time-aware warp, pinned to the REFERENCE's own code by composition.  Runs only
where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_warp_voxel.py

The reference documents a voxel motion model (src/warp.py:199, 211) and ships without its branch (:223-228), so there is no output of
its own to record.  What a voxel warp MUST be is fixed all the same: the events of time bin k, warped by the reference's
``Warp(normalize_t=False).warp_event_from_optical_flow(events_k, voxel[k], reference_time)`` with the reference time of the WHOLE
window (``calculate_reftime``), scattered back to input order.  Windows whose times span exactly [0, 1] pin ``normalize_t=True`` as
well: the period is exactly 1 for every direction, and dividing by it changes nothing.  The IWE: the reference's
``bilinear_vote_tensor`` of those warped events, float64.  Only the bin rule (float64, ``k = min(int(tau T), T - 1)``) is written
here, in numpy; tests/test_warp_voxel.py checks it on its edge cases by hand.

Cases (image 5 x 7, n = 200, every bin's flow different):
  ev_<w>_<b>             events float64 [b, n, 4] of window w ("unit": times span [0, 1]; "sec": [0.25, 3.75]), b rows
  vox_<T>_<b>            voxel float64 [b, T, 2, 5, 7]
  warp_<w>_<b>_<T>_<d>_<np|t64|t32>   warped [b, n, 4]; d indexes DIRECTIONS; the combinations ``cases()`` lists
  iwe_<T>_<pad>[_w]      float64 IWE of window "unit" row 0, direction "middle", outer padding pad, unit | per-event weights (iwe_weight)
"""
import os
import sys
import warnings

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True

H, W, N = 5, 7, 200
BINS = (1, 2, 3, 5)
DIRECTIONS = ("first", "middle", "last", 0.3, "before", "after")
WINDOWS = {"unit": (0.0, 1.0), "sec": (0.25, 3.5)}


def cases():
    """(window, b, T, index into DIRECTIONS, container): every T and direction in every container on the un-batched unit window; fewer
    on the window in seconds and on the batched ones (a committed fixture stays small)."""
    for T in BINS:
        for d in range(len(DIRECTIONS)):
            for tag in ("np", "t64", "t32"):
                yield "unit", 1, T, d, tag
        for d in (0, 3, 5):
            for tag in ("t64", "t32"):
                yield "sec", 1, T, d, tag
    for w in WINDOWS:
        for T in (2, 5):
            for d in (1, 3):
                for tag in ("t64", "t32"):
                    yield w, 2, T, d, tag


def events(window: str, b: int) -> np.ndarray:
    t0, span = WINDOWS[window]
    rs = np.random.RandomState(4200 + 10 * b + len(window))
    ev = np.empty((b, N, 4))
    ev[..., 0] = rs.uniform(0.0, H - 1e-3, (b, N))
    ev[..., 1] = rs.uniform(0.0, W - 1e-3, (b, N))
    ev[..., 2] = t0 + span * rs.uniform(0.0, 1.0, (b, N))
    ev[..., 3] = rs.randint(0, 2, (b, N))
    exact = [0.0, 1.0, 0.5, 0.25, 0.75, 0.2, 0.4, 0.6, 0.8, 1.0 / 3.0, 2.0 / 3.0]      # tmin, tmax and bin boundaries
    for r in range(b):
        at = rs.permutation(N)[:len(exact)]
        ev[r, at, 2] = t0 + span * np.array(exact)
        ev[r, :5, :2] = np.floor(ev[r, :5, :2])                                           # some integer coordinates
    return ev


def voxel(T: int, b: int) -> np.ndarray:
    return np.random.RandomState(4300 + 10 * T + b).uniform(-1.5, 1.5, (b, T, 2, H, W))


def bins_of(t: np.ndarray, T: int) -> np.ndarray:
    t = t.astype(np.float64)
    span = t.max() - t.min()
    if not span > 0:
        return np.zeros(t.shape, dtype=np.int64)
    return np.minimum((((t - t.min()) / span) * float(T)).astype(np.int64), T - 1)


def compose(ref_warp, ev, vx, direction):
    """One window [n, 4], one voxel [T, 2, H, W] (arrays or tensors of one dtype) -> warped [n, 4] by the reference, bin by bin."""
    is_t = isinstance(ev, torch.Tensor)
    T = vx.shape[0]
    k = bins_of(ev[:, 2].numpy() if is_t else ev[:, 2], T)
    ref_time = ref_warp.calculate_reftime(ev, direction)
    out = ev.clone() if is_t else ev.copy()
    for b in range(T):
        at = np.nonzero(k == b)[0]
        if len(at) == 0:
            continue
        sel = torch.from_numpy(at) if is_t else at
        part = ev[sel].clone() if is_t else ev[sel].copy()
        warped, _ = ref_warp.warp_event_from_optical_flow(part, vx[b], ref_time)
        out[sel] = warped.reshape(len(at), 4)
    return out


def main():
    sys.path.insert(0, REF)
    from src.event_image_converter import EventImageConverter
    from src.warp import Warp

    ref_warp = Warp((H, W), normalize_t=False)
    out = {}
    for w, b, T, d, tag in cases():
        ev = out.setdefault(f"ev_{w}_{b}", events(w, b))
        vx = out.setdefault(f"vox_{T}_{b}", voxel(T, b))
        conv = {"np": lambda a: a.copy(), "t64": lambda a: torch.from_numpy(a.copy()),
                "t32": lambda a: torch.from_numpy(a.astype(np.float32))}[tag]
        rows = [compose(ref_warp, conv(ev[r]), conv(vx[r]), DIRECTIONS[d]) for r in range(b)]
        out[f"warp_{w}_{b}_{T}_{d}_{tag}"] = np.stack([np.asarray(r) for r in rows])
    weight = out["iwe_weight"] = np.random.RandomState(4400).uniform(0.2, 2.0, N)
    ev = torch.from_numpy(out["ev_unit_1"][0])
    for T in BINS:
        warped = compose(ref_warp, ev, torch.from_numpy(out[f"vox_{T}_1"][0]), "middle")
        for pad in (0, 2):
            conv = EventImageConverter((H, W), outer_padding=pad)
            out[f"iwe_{T}_{pad}"] = conv.bilinear_vote_tensor(warped).numpy()
            out[f"iwe_{T}_{pad}_w"] = conv.bilinear_vote_tensor(warped, torch.from_numpy(weight)).numpy()
    path = os.path.join(HERE, "golden_warp_voxel.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(out)} arrays")


if __name__ == "__main__":
    main()
