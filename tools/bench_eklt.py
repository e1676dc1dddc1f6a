#!/usr/bin/env python3
"""Benchmark of the sampled EKLT sweep (csrc/eklt_sweep.hip, solver/eklt_sweep.py) against the same sweep as eager torch float64 on
the same GPU and against the numpy restatement on the host.

    python tools/bench_eklt.py --out profiles/eklt_bench.json [--sizes 260x346 720x1280] [--k 800]

Per size (260 x 346 and 720 x 1280, the reference YAML's options with the velocity model and a translation within 0.4 px, ROI = the
central half of the columns) and per patch geometry (patch 4 / slide 2 and patch 32 / slide 32), K hypotheses:
  hip_ms             ``ebos_eklt_sweep_batch_f64`` (selection norms, sweep, argmin; no cost table stored), device events around
                     the call; warm-up, then 5 rounds alternating with the torch sweep; best and all rounds;
  hip_window_ms      one ``estimate`` (upload, splat, prepare pass, selection, sweep, flow, read-back), host clock, best of 3;
  torch_gpu_ms       the same P x K costs in eager torch float64 on the same GPU: per hypothesis the whole image warped by shifted
                     slices, the patches taken with ``unfold`` (zero-padded to whole boxes, which changes no norm and no column
                     sum), norms, column sums, maximum, running argmin -- batched over patches, a loop over hypotheses (a
                     [P, K, p, p] float64 batch over hypotheses too would hold 11.8 GB at 720 x 1280, patch 4 / slide 2);
  numpy_ms_scaled    tests/_eklt_ref.py on the host for the first ``numpy_boxes`` scored boxes x ``numpy_hyp`` hypotheses, scaled
                     to P x K (the whole-image warp of a hypothesis is computed once and shared by the boxes, as in the table);
  evaluations_per_s  P_scored x K / hip time; flop_per_eval counts the float64 operations of one (box, hypothesis) evaluation --
                     two passes of 8 products + 6 sums for the warp of gx and gy, 2 products + 1 sum for P0, then square + add (pass 1) or
                     divide + subtract + abs + add (pass 2, the division counted once) per pixel -- and fp64_share is their rate
                     against the MI355X's published float64 vector peak of 78.6 TFLOP/s (half its 157.3 TFLOP/s float32 vector peak).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _eklt_ref as E  # noqa: E402
from _eklt_warp64 import shift_and_weights  # noqa: E402
from _gml_cases import YAML_GML, frame_image, synth_events  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12
FLOP_PER_PIXEL = 2 * (14 + 3) + 2 + 4   # 40
PARAMS = {"v_x": {"min": -1.0, "max": 1.0}, "v_y": {"min": -1.0, "max": 1.0}, "p_x": {"min": -0.4, "max": 0.4},
          "p_y": {"min": -0.4, "max": 0.4}}


def config(H, W, patch, slide, k):
    gml = dict(YAML_GML)
    gml.update({"poisson_model": False, "weight_loss_by_inverse_event_hist": False, "angle_model": False, "optimize_warp": True})
    return {"method": "patch_eklt", "filter": {"filters": [], "parameters": {"xmin": 0, "xmax": H, "ymin": W // 4, "ymax": W - W // 4}},
            "cost_with_weight": {"diff_norm": 1.0}, "generative_ml": gml,
            "optimizer": {"method": "optuna", "sampler": "random", "n_iter": k, "parameters": PARAMS},
            "patch_eklt": {"patch_size": patch, "sliding_window": slide, "do_event_thresholding": False, "event_thres": 8}}


def torch_sweep(gx, gy, q, sel, hyp4, p, s, gh, gw):
    """-> (best cost [gh gw], best index [gh gw]) over the selected boxes; everything float64 on gx's device."""
    H, W = gx.shape
    eh, ew = (gh - 1) * s + p, (gw - 1) * s + p            # the grid's extent: the last boxes may pass the image's edge
    pad_to = lambda a: F.pad(a, (0, ew - W, 0, eh - H))
    boxes = lambda a: pad_to(a).unfold(0, p, s).unfold(1, p, s).reshape(gh * gw, p, p)
    Q = boxes(q)
    Q = Q / torch.linalg.norm(Q.reshape(gh * gw, -1), dim=1)[:, None, None]
    h = 2
    gxp, gyp = F.pad(gx, (h, h, h, h)), F.pad(gy, (h, h, h, h))
    best = torch.full((gh * gw,), float("inf"), dtype=torch.float64, device=gx.device)
    best_k = torch.full((gh * gw,), -1, dtype=torch.int64, device=gx.device)
    for k, (vx, vy, px, py) in enumerate(hyp4):
        sr, sc, (w00, w01, w10, w11) = shift_and_weights(px, py)
        at = lambda g, dr, dc: g[h + sr + dr:h + sr + dr + H, h + sc + dc:h + sc + dc + W]
        warp = lambda g: ((at(g, 0, 0) * w00 + at(g, 0, 1) * w01) + at(g, 1, 0) * w10) + at(g, 1, 1) * w11
        P = boxes(vx * warp(gxp) + vy * warp(gyp))
        P = P / (torch.linalg.norm(P.reshape(gh * gw, -1), dim=1) + 1e-4)[:, None, None]
        cost = (P - Q).abs().sum(1).max(1).values
        better = sel & (cost < best)
        best = torch.where(better, cost, best)
        best_k = torch.where(better, torch.full_like(best_k, k), best_k)
    return best, best_k


def bench(H, W, patch, slide, K, rounds=5, numpy_boxes=8, numpy_hyp=16):
    import event_based_bos_amd as ebos
    from event_based_bos_amd._hip import check, ptr, stream_ptr

    lib = ebos._hip.require_gpu()
    dev = torch.device("cuda:0")
    cfg = config(H, W, patch, slide, K)
    frame, events = frame_image(H, W, 1), synth_events(2 * H * W, H, W, 2)
    solv = ebos.solver.GenerativePatchIndependent((H, W), (H, W), {}, cfg)
    out = {"size": [H, W], "patch": patch, "slide": slide, "hypotheses": K, "boxes": int(solv.n_patch)}
    # one window through the public call
    np.random.seed(0)
    solv.estimate(events, frame=frame)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        np.random.seed(0)
        t0 = time.perf_counter()
        solv.estimate(events, frame=frame)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    out["hip_window_ms"], out["hip_window_ms_all"] = min(ts), ts
    scored = solv.estimate_indices
    out["boxes_scored"] = int(len(scored))
    # the sweep alone, on the restatement's planes
    roi = solv._gml_roi
    st = E.state(frame, events, cfg["generative_ml"], roi)
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    gx, gy, q = t(st["gx"]), t(st["gy"]), t(st["hist"] / np.linalg.norm(st["hist"]))
    np.random.seed(0)
    hyp4 = ebos.solver.eklt_sweep.unfold_table(cfg["generative_ml"], list(PARAMS), solv.hypothesis_table())
    gh, gw = solv.patch_image_size
    sel_np = np.zeros(gh * gw, dtype=np.int32)
    sel_np[scored] = 1
    sel, boxes = t(sel_np, torch.int32), t(solv._eklt_boxes, torch.int32)
    ph, pw = solv._eklt_box_bound
    halo = int(lib.ebos_eklt_sweep_halo(hyp4.ctypes.data, K))
    route = ebos._hip.EKLT_ROUTE_PATCH if lib.ebos_eklt_sweep_fits(ph, pw, halo) else ebos._hip.EKLT_ROUTE_ROI
    out["route"], out["halo"] = ("patch" if route == ebos._hip.EKLT_ROUTE_PATCH else "roi"), halo
    nbytes = int(lib.ebos_eklt_sweep_scratch_bytes(1, gh * gw, K, route))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    best_cost = torch.empty(gh * gw, dtype=torch.float64, device=dev)
    best_index = torch.empty(gh * gw, dtype=torch.int32, device=dev)

    def hip():
        check(lib.ebos_eklt_sweep_batch_f64(1, H, W, ptr(gx), ptr(gy), 0, ptr(q), None, ptr(boxes), gh * gw, ph, pw, ptr(sel),
                                            hyp4.ctypes.data, K, 0, 1.0, route, None, ptr(best_cost), ptr(best_index), ptr(scratch),
                                            nbytes, stream_ptr(dev)), "ebos_eklt_sweep_batch_f64")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    eager = lambda: torch_sweep(gx, gy, q, sel.bool(), hyp4, patch, slide, gh, gw)
    hip()
    eager()
    torch.cuda.synchronize()
    hip_ms, torch_ms = [], []
    for _ in range(rounds):
        hip_ms.append(timed(hip)[0])
        ms, (tb, tk) = timed(eager)
        torch_ms.append(ms)
    out["hip_ms"], out["hip_ms_all"] = min(hip_ms), hip_ms
    out["torch_gpu_ms"], out["torch_gpu_ms_all"] = min(torch_ms), torch_ms
    out["torch_over_hip"] = min(torch_ms) / min(hip_ms)
    same = (best_index.long() == tk)
    out["winners_equal_torch"] = float(same.double().mean())
    out["best_cost_max_abs_diff_vs_torch"] = float((best_cost - tb)[sel.bool() & same].abs().max())
    n_box = int(np.prod(solv._eklt_box_bound))
    evals = len(scored) * K
    out["evaluations"] = evals
    out["evaluations_per_s"] = evals / (min(hip_ms) * 1e-3)
    out["flop_per_eval"] = FLOP_PER_PIXEL * n_box
    out["fp64_share"] = out["evaluations_per_s"] * out["flop_per_eval"] / FP64_VECTOR_PEAK
    # numpy on the host: a sample, scaled
    nb, nh = min(numpy_boxes, len(scored)), min(numpy_hyp, K)
    t0 = time.perf_counter()
    E.cost_table(st, cfg["generative_ml"], solv._eklt_boxes[scored[:nb]], hyp4[:nh], 1.0)
    dt = time.perf_counter() - t0
    out["numpy_sample"] = [nb, nh]
    out["numpy_ms_scaled"] = 1e3 * dt * evals / (nb * nh)
    out["numpy_over_hip"] = out["numpy_ms_scaled"] / min(hip_ms)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["260x346", "720x1280"])
    ap.add_argument("--geometries", nargs="+", default=["4/2", "32/32"], help="patch/slide")
    ap.add_argument("--k", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "runs": []}
    for size in args.sizes:
        H, W = (int(v) for v in size.split("x"))
        for geo in args.geometries:
            p, s = (int(v) for v in geo.split("/"))
            r = bench(H, W, p, s, args.k, args.rounds)
            print(json.dumps(r), flush=True)
            res["runs"].append(r)
            if args.out:   # after every run: a long benchmark leaves what it has
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
