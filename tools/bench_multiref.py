"""Measure the multi-reference contrast at K = 3, directions [first, middle, last]: forward alone and forward +
backward of the variance contrast, for three contenders in one process, alternating, best of ``--rounds`` rounds, warmed up, with a
device synchronise inside the clock:

    (a) fused   EventPlan.iwe_dense_multi / contrast_dense_multi(fused=True): one pass over the events, the owner backward
    (b) loop    the same operators with fused=False: K calls of the tiled forward and of the atomic backward on dt + shift_k
    (c) plans   what a caller could do before these operators: three plans, one per direction, each through iwe_dense /
                variance_and_grad_dense (the slab pipeline), the gradients added

    python tools/bench_multiref.py [--out profiles/multiref_bench.json] [--rounds 5] [--reps 20]

Reports each best and its max - min spread over the rounds; a difference counts only where the intervals [best, best + spread] lie
apart.  Prints one JSON document."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import event_based_bos_amd as ebos  # noqa: E402

DIRECTIONS = ["first", "middle", "last"]
CASES = [("2M@1280x720", 2_000_000, (720, 1280)), ("100k@346x260", 100_000, (260, 346))]
CONFIGS = [(64, 64, 16), (32, 32, 32)]


def synth(n, shape, seed=0):
    """Integer sensor coordinates, times sorted on [0, 1]; a smooth flow of a few pixels (BOS displacements are small)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    H, W = shape
    ev = torch.stack([torch.randint(0, H, (n,), generator=g).double(), torch.randint(0, W, (n,), generator=g).double(),
                      torch.sort(torch.rand(n, generator=g, dtype=torch.float64)).values, torch.randint(0, 2, (n,), generator=g).double()], 1)
    ev[0, 2], ev[-1, 2] = 0.0, 1.0
    coarse = (torch.rand((1, 2, 6, 8), generator=g) * 2 - 1) * 3.0
    flow = torch.nn.functional.interpolate(coarse, size=shape, mode="bicubic", align_corners=False)[0].contiguous()
    return ev.cuda(), flow.cuda()


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def measure(contenders, rounds, reps):
    for fn in contenders.values():   # warm-up: workspaces, jobs, the shifted dt of the loop route
        for _ in range(3):
            fn()
    samples = {k: [] for k in contenders}
    for _ in range(rounds):
        for k, fn in contenders.items():
            samples[k].append(timed(fn, reps))
    return {k: {"best_us": round(min(v), 2), "spread_us": round(max(v) - min(v), 2), "rounds_us": [round(x, 2) for x in v]}
            for k, v in samples.items()}


def run_case(name, n, shape, tile_h, tile_w, halo, rounds, reps):
    ev, flow = synth(n, shape)
    plan = ebos.EventPlan.build(ev, shape, "first", True, tile=(tile_h, tile_w), emit="full")
    plans = [ebos.EventPlan.build(ev, shape, d, True, tile=(tile_h, tile_w), emit="full") for d in DIRECTIONS]
    leaf = flow.clone().requires_grad_(True)

    def fwd(fused):
        with torch.no_grad():
            return plan.iwe_dense_multi(flow, DIRECTIONS, halo=halo, fused=fused)

    def fwd_bwd(fused):
        leaf.grad = None
        v = plan.contrast_dense_multi(leaf, DIRECTIONS, halo=halo, fused=fused)
        v.backward()
        return v.detach(), leaf.grad

    def plans_fwd():
        with torch.no_grad():
            return torch.stack([p.iwe_dense(flow, halo=halo) for p in plans])

    def plans_fwd_bwd():
        out = [p.variance_and_grad_dense(flow, halo=halo) for p in plans]
        return sum(v for v, _ in out) / len(out), sum(g for _, g in out) / len(out)

    # the contenders compute the same thing
    ia, ib, ic = fwd(True), fwd(False), plans_fwd()
    (va, ga), (vb, gb), (vc, gc) = fwd_bwd(True), fwd_bwd(False), plans_fwd_bwd()
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    agree = {"iwe_fused_vs_plans": rel(ia, ic), "iwe_loop_vs_plans": rel(ib, ic), "value_fused_vs_plans": abs(float(va) - float(vc)) / float(vc),
             "grad_fused_vs_plans": rel(ga, gc), "grad_loop_vs_plans": rel(gb, gc)}
    # (the images are continuous in dt; a gradient is not -- an event whose float32 dt_k and a plan's own dt differ in the last
    # bit may sit on either side of a kink of the vote --, so the gradients' agreement is recorded, not judged)
    assert max(agree["iwe_fused_vs_plans"], agree["iwe_loop_vs_plans"], agree["value_fused_vs_plans"]) < 1e-3, agree
    res = {"case": name, "events": n, "image": list(shape), "tile": [tile_h, tile_w], "halo": halo, "K": len(DIRECTIONS),
           "fits": int(ebos.load_library().ebos_iwe_multiref_fits(tile_h, tile_w, halo, len(DIRECTIONS))), "agreement": agree,
           "forward": measure({"fused": lambda: fwd(True), "loop": lambda: fwd(False), "plans": plans_fwd}, rounds, reps),
           "forward_backward": measure({"fused": lambda: fwd_bwd(True), "loop": lambda: fwd_bwd(False), "plans": plans_fwd_bwd},
                                       rounds, reps)}
    for p in [plan] + plans:
        p.clear_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ebos.load_library()
    results = [run_case(name, n, shape, th, tw, hl, args.rounds, args.reps) for name, n, shape in CASES for th, tw, hl in CONFIGS]
    doc = {"tool": "tools/bench_multiref.py", "device": torch.cuda.get_device_name(0), "directions": DIRECTIONS, "rounds": args.rounds,
           "reps": args.reps, "unit": "microseconds per call, device synchronise inside the clock", "results": results}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
