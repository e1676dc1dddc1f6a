"""Measure the K-image slab pipeline of the multi-reference contrast and the native multi-reference Adam loop at K = 3,
directions [first, middle, last], in one process, the contenders alternating, best of ``--rounds`` rounds, warmed up, with a device
synchronise inside the clock (the protocol of tools/bench_multiref.py):

    (a) operator, forward alone and forward + backward of the variance contrast
        slab         EventPlan.iwe_dense_multi / contrast_dense_multi(fused="slab"): the K-image slab forward, the K-reference
                     tile-private backward, through autograd
        slab_direct  EventPlan.variance_multi_value_and_grad: the same three launches without autograd (forward + backward only)
        loop         the same operators with fused=False: K calls of the tiled forward and of the atomic backward on dt + shift_k
        plans        three plans, one per direction, each through iwe_dense / variance_and_grad_dense (the single slab pipeline)
    (b) per Adam iteration of the patch-flow solver
        native       solver/multi_reference_loop.MultiReferencePatchLoop: ``--reps`` iterations per C call
        autograd     the existing multi-reference autograd loop of ContrastMaximization (fused: false, torch.optim.Adam)
        single       the SINGLE-reference native loop, four launches per iteration (fused_loop.FusedPatchLoop, resident off): the floor

    python tools/bench_multiref_loop.py [--out profiles/multiref_loop_bench.json] [--rounds 5] [--reps 20]

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
from event_based_bos_amd import ops  # noqa: E402
from event_based_bos_amd.solver import fused_loop  # noqa: E402
from event_based_bos_amd.solver.multi_reference_loop import MultiReferencePatchLoop  # noqa: E402

DIRECTIONS = ["first", "middle", "last"]
CASES = [("2M@1280x720", 2_000_000, (720, 1280), (24, 32)), ("100k@346x260", 100_000, (260, 346), (20, 26))]
CONFIGS = [(64, 64, 16), (32, 32, 32)]


def synth(n, shape, seed=0):
    """Integer sensor coordinates, times sorted on [0, 1]; a smooth flow of a few pixels (tools/bench_multiref.py)."""
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


def measure(contenders, rounds, reps, per_call=1):
    """``per_call``: iterations one call of a contender runs (the loops enqueue ``reps`` iterations per call and are called once)."""
    for fn in contenders.values():
        for _ in range(3):
            fn()
    samples = {k: [] for k in contenders}
    for _ in range(rounds):
        for k, fn in contenders.items():
            samples[k].append(timed(fn, reps) / per_call)
    return {k: {"best_us": round(min(v), 2), "spread_us": round(max(v) - min(v), 2), "rounds_us": [round(x, 2) for x in v]}
            for k, v in samples.items()}


def run_operator(name, n, shape, tile_h, tile_w, halo, rounds, reps):
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

    def direct():
        return plan.variance_multi_value_and_grad(flow, DIRECTIONS, halo=halo)

    def plans_fwd():
        with torch.no_grad():
            return torch.stack([p.iwe_dense(flow, halo=halo) for p in plans])

    def plans_fwd_bwd():
        out = [p.variance_and_grad_dense(flow, halo=halo) for p in plans]
        return sum(v for v, _ in out) / len(out), sum(g for _, g in out) / len(out)

    # the contenders compute the same thing
    ia, ib, ic = fwd("slab"), fwd(False), plans_fwd()
    (va, ga), (vb, gb), (vc, gc), (vd, gd) = fwd_bwd("slab"), fwd_bwd(False), plans_fwd_bwd(), direct()
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    agree = {"iwe_slab_vs_plans": rel(ia, ic), "iwe_loop_vs_plans": rel(ib, ic), "value_slab_vs_plans": abs(float(va) - float(vc)) / float(vc),
             "grad_slab_vs_plans": rel(ga, gc), "grad_loop_vs_plans": rel(gb, gc), "grad_slab_direct_vs_slab": rel(gd, ga)}
    # (a gradient is not continuous in dt -- an event whose float32 dt_k and a plan's own dt differ in the last bit may sit on either
    # side of a kink of the vote --, so the gradients' agreement with the three plans is recorded, not judged)
    assert max(agree["iwe_slab_vs_plans"], agree["iwe_loop_vs_plans"], agree["value_slab_vs_plans"]) < 1e-3, agree
    assert torch.equal(gd, ga) and float(vd) == float(va), agree
    res = {"case": name, "events": n, "image": list(shape), "tile": [tile_h, tile_w], "halo": halo, "K": len(DIRECTIONS), "agreement": agree,
           "forward": measure({"slab": lambda: fwd("slab"), "loop": lambda: fwd(False), "plans": plans_fwd}, rounds, reps),
           "forward_backward": measure({"slab": lambda: fwd_bwd("slab"), "slab_direct": direct, "loop": lambda: fwd_bwd(False),
                                        "plans": plans_fwd_bwd}, rounds, reps)}
    for p in [plan] + plans:
        p.clear_cache()
    return res


def run_solver(name, n, shape, patch, tile_h, tile_w, halo, rounds, reps):
    ev, _ = synth(n, shape)
    H, W = shape
    cfg = {"motion_model": "dense-flow", "warp_direction": "first", "cost": "image_variance", "outer_padding": 0, "halo": halo,
           "tile": [tile_h, tile_w], "patch": {"size": list(patch), "sliding_window": list(patch)},
           "optimizer": {"method": "Adam", "n_iter": reps, "parameters": {"lr": 0.05}, "fused": False, "graph": False},
           "multi_reference": {"directions": DIRECTIONS, "fused": False}}
    slv = ebos.solver.collections["contrast_maximization"](shape, shape, solver_config=cfg)
    plan = ebos.EventPlan.build(ev, shape, "first", True, tile=(tile_h, tile_w), emit="full")
    lean = ebos.EventPlan.build(ev, shape, "first", True, tile=(tile_h, tile_w), emit="compact")
    gh, gw = ebos.solver.contrast_maximization.patch_grid_shape(shape, patch, patch)
    g = torch.Generator(device="cpu").manual_seed(3)
    theta0 = ((torch.rand((2, gh, gw), generator=g) * 2 - 1) * 2.0).cuda()
    capacity = (rounds + 4) * reps
    native = MultiReferencePatchLoop(plan, patch, patch, theta0, DIRECTIONS, halo=halo, capacity=capacity)
    single = fused_loop.FusedPatchLoop(lean, patch, patch, theta0.clone(), 1.0, halo=halo, capacity=capacity)
    theta = theta0.clone().requires_grad_(True)
    opt = torch.optim.Adam([theta], lr=0.05)

    def autograd_iteration():
        opt.zero_grad(set_to_none=True)
        loss = slv.objective(plan, ops.upsample_patch_flow(theta, patch, patch, (H, W)))
        loss.backward()
        opt.step()

    def autograd_call():
        with torch.autograd.set_multithreading_enabled(False):   # as ContrastMaximization.estimate runs its loop
            for _ in range(reps):
                autograd_iteration()

    # the first losses agree (the same objective from the same start)
    first_native = float(MultiReferencePatchLoop(plan, patch, patch, theta0, DIRECTIONS, halo=halo, capacity=1).solve(1)[0])
    with torch.no_grad():
        first_autograd = float(slv.objective(plan, ops.upsample_patch_flow(theta0, patch, patch, (H, W))))
    assert abs(first_native - first_autograd) < 1e-4 * abs(first_autograd), (first_native, first_autograd)
    # one call = ``reps`` iterations, timed once per round
    timing = measure({"native": lambda: native.solve(reps), "autograd": autograd_call, "single": lambda: single.run(reps, resident=False)},
                     rounds=rounds, reps=1, per_call=reps)   # (3 warm-up calls + ``rounds`` timed ones: inside ``capacity``)
    res = {"case": name, "events": n, "image": list(shape), "tile": [tile_h, tile_w], "halo": halo, "K": len(DIRECTIONS), "patch": list(patch),
           "iterations_per_call": reps, "first_loss": {"native": first_native, "autograd": first_autograd}, "per_iteration": timing}
    plan.clear_cache()
    lean.clear_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ebos.load_library()
    operator = [run_operator(name, n, shape, th, tw, hl, args.rounds, args.reps) for name, n, shape, _ in CASES for th, tw, hl in CONFIGS]
    solver = [run_solver(name, n, shape, patch, th, tw, hl, args.rounds, args.reps) for name, n, shape, patch in CASES for th, tw, hl in CONFIGS]
    doc = {"tool": "tools/bench_multiref_loop.py", "device": torch.cuda.get_device_name(0), "directions": DIRECTIONS, "rounds": args.rounds,
           "reps": args.reps, "unit": "microseconds per call (operator) / per Adam iteration (solver), device synchronise inside the clock",
           "operator": operator, "solver": solver}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
