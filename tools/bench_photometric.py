#!/usr/bin/env python3
"""Timing of the photometric check (event_based_bos_amd/photometric.py, csrc/photometric.hip).

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ph -- python tools/bench_photometric.py --kernels-only
    python tools/bench_photometric.py --kernel-trace <dir>/.../ph_kernel_trace.csv [--out profiles/photometric_bench.json]

Shapes 720 x 1280 and 260 x 346, B = 1 and 8, uint8 frames, float32 flows.  Per shape, in one process, alternated round by round
(best of ``--rounds`` rounds, with the spread): the fused score (``photometric_error_batch``: two launches), the kernels alone
(``warp_image_forward_batch``, ``ssim_map``, ``ssim`` = the map plus its means) and an eager-torch statement of the same score on
the same GPU (``grid_sample`` + ``conv2d`` + masked sums).  Times are device events around ``--reps`` calls.

Kernel times come from a ``rocprofv3 --kernel-trace`` run of its own (``--kernels-only`` launches every entry a few times per
shape); ``--kernel-trace`` reads its per-dispatch CSV and groups the dispatches by kernel and grid.  Next to each kernel time stand
the bytes and multiply-adds the algorithm needs, computed from the shapes, the least time the hardware could take for either (8 TB/s,
157.3 TFLOP/s of float32 vector rate at 2 FLOP per multiply-add) and which of the two bounds the kernel.
"""
import argparse
import csv
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from event_based_bos_amd import photometric as ph  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
FP32_FLOP_PER_S = 157.3e12
SHAPES = ((720, 1280), (260, 346))
BATCHES = (1, 8)
WS = 11


def inputs(B, H, W, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.rand((B, 1, H + 2, W + 2), device="cuda", generator=g)
    frame1 = (F.avg_pool2d(base, 3, stride=1)[:, 0] * 255).round().to(torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                            indexing="ij")
    flow = torch.stack([1.3 * torch.sin(yy / 37.0) * torch.cos(xx / 53.0) + 0.31, 0.9 * torch.cos(yy / 41.0) * torch.sin(xx / 29.0) - 0.27])
    flow = flow[None].repeat(B, 1, 1, 1).contiguous()
    frame2 = ph.warp_image_forward_batch(frame1, flow).round().clamp(0, 255).to(torch.uint8)
    return frame1, frame2, flow


def eager_score(frame1, frame2, flow, taps):
    """The score of photometric_error_batch in eager torch: [B, 7]."""
    B, H, W = frame2.shape
    f1, f2 = frame1.float(), frame2.float()
    kh, kw = (H - 1) / 2.0, (W - 1) / 2.0
    rows, cols = torch.meshgrid(torch.arange(H, device=flow.device), torch.arange(W, device=flow.device), indexing="ij")
    nr, nc = (rows / kh - 1) - flow[:, 0] / kh, (cols / kw - 1) - flow[:, 1] / kw
    w = F.grid_sample(f1[:, None], torch.stack([nc, nr], dim=-1), mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    r0, c0 = torch.floor((nr + 1) * kh), torch.floor((nc + 1) * kw)
    ok = (r0 >= 0) & (r0 + 1 <= H - 1) & (c0 >= 0) & (c0 + 1 <= W - 1) & torch.isfinite(flow).all(dim=1)
    n = ok.sum(dim=(1, 2)).double()
    k = taps[None, None]

    def ssim_map(a, b):
        conv = lambda x: F.conv2d(x[:, None], k, padding=WS // 2)[:, 0]
        mu1, mu2 = conv(a), conv(b)
        s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
        return ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))

    out = []
    for x in (w, f1):
        d = (x - f2) * ok
        out += [d.abs().double().sum(dim=(1, 2)) / n, torch.sqrt((d * d).double().sum(dim=(1, 2)) / n),
                (ssim_map(x, f2) * ok).double().sum(dim=(1, 2)) / n]
    return torch.stack(out + [n], dim=1)


def variants(B, H, W):
    frame1, frame2, flow = inputs(B, H, W)
    a, b = frame1.float()[:, None].contiguous(), frame2.float()[:, None].contiguous()
    taps = ph.window_taps(WS).cuda()
    return {
        "fused_score": lambda: ph.photometric_error_batch(frame1, frame2, flow),
        "warp_alone": lambda: ph.warp_image_forward_batch(frame1, flow),
        "ssim_map_alone": lambda: ph.ssim_map(a, b),
        "ssim_with_means": lambda: ph.ssim(a, b, size_average=False),
        "eager_torch_score": lambda: eager_score(frame1, frame2, flow, taps),
    }, (frame1, frame2, flow, taps)


def time_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # microseconds per call


def algorithm(B, H, W):
    """Bytes and multiply-adds the kernels need, from the shapes (uint8 frames, float32 flow and maps)."""
    px = B * H * W
    madds_ssim = 5 * WS * WS * px
    need = {
        "warp_image_kernel": {"bytes": px * (1 + 8 + 4), "multiply_adds": 8 * px},
        "ssim_map_kernel": {"bytes": px * 12, "multiply_adds": madds_ssim},
        "photometric_tiles": {"bytes": px * (1 + 1 + 8), "multiply_adds": 2 * madds_ssim + 8 * px},
    }
    for v in need.values():
        t_mem, t_alu = v["bytes"] / HBM_BYTES_PER_S, 2 * v["multiply_adds"] / FP32_FLOP_PER_S
        v["least_us"] = max(t_mem, t_alu) * 1e6
        v["bound"] = "memory (8 TB/s)" if t_mem >= t_alu else "float32 vector rate (157.3 TFLOP/s; the unfused multiply-adds reach half of it)"
    return need


def tiles(H, W):
    return ((W + 63) // 64) * ((H + 15) // 16)


def read_trace(path):
    """{(short kernel name, grid x, grid y): [durations in ns]} of a rocprofv3 kernel-trace CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            short = next((k for k in ("warp_image_kernel", "ssim_map_kernel", "photometric_tiles",
                                      "photometric_finish") if k in name), None)
            if short is None:
                continue
            key = (short, int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]))
            out.setdefault(key, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return out


def kernel_rows(trace, B, H, W):
    """The traced kernels of one shape: the grid of each is known from the shape."""
    t = tiles(H, W) * 256
    warp_grid = min((H * W + 255) // 256, 2048) * 256
    want = {"warp_image_kernel": (warp_grid, B), "ssim_map_kernel": (t, B), "photometric_tiles": (t, B),
            "photometric_finish": (B * 256, 1)}
    need = algorithm(B, H, W)
    rows = {}
    for name, (gx, gy) in want.items():
        d = sorted(trace.get((name, gx, gy), []))
        if not d:
            rows[name] = "NOT YET MEASURED"
            continue
        d = d[:len(d) - len(d) // 5]     # (without the slowest fifth: the first, cold dispatches)
        row = {"dispatches": len(d), "median_us": d[len(d) // 2] / 1e3, "min_us": d[0] / 1e3, "max_us": d[-1] / 1e3}
        if name in need:
            row.update(need[name])
            row["share_of_least_time"] = need[name]["least_us"] / row["median_us"]
        rows[name] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="only launch every entry a few times per shape, for a rocprofv3 kernel trace")
    ap.add_argument("--kernel-trace", default=None, help="the kernel-trace CSV of a rocprofv3 run of `--kernels-only`")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_photometric needs a GPU"
    trace = read_trace(args.kernel_trace) if args.kernel_trace else None
    res = {"device": torch.cuda.get_device_name(0), "window_size": WS, "frames": "uint8", "flow": "float32", "reps": args.reps,
           "rounds": args.rounds, "note": "us per call from device events around `reps` calls; best of `rounds` rounds, the variants "
           "alternated within a round; kernels: a rocprofv3 --kernel-trace run of its own", "shapes": []}
    for H, W in SHAPES:
        for B in BATCHES:
            fns, (frame1, frame2, flow, taps) = variants(B, H, W)
            if args.kernels_only:
                for name, fn in fns.items():
                    if name != "eager_torch_score":
                        for _ in range(12):
                            fn()
                torch.cuda.synchronize()
                continue
            table = fns["fused_score"]()[0]
            eager = fns["eager_torch_score"]()
            for fn in fns.values():     # warm every variant at this shape
                fn()
            torch.cuda.synchronize()
            rounds = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    rounds[k].append(time_call(fn, args.reps))
            row = {"H": H, "W": W, "B": B, "n_points": float(table[0, 6]),
                   "fused_vs_eager_max_abs_difference": float((table[:, :6] - eager[:, :6]).abs().max()),
                   "us_per_call": {k: {"best": min(v), "worst": max(v), "spread": (max(v) - min(v)) / min(v)} for k, v in rounds.items()}}
            row["fused_over_eager"] = row["us_per_call"]["fused_score"]["best"] / row["us_per_call"]["eager_torch_score"]["best"]
            row["kernels"] = kernel_rows(trace, B, H, W) if trace is not None else "NOT YET MEASURED"
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
