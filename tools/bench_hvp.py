"""Measure the contrast's Hessian-vector product on tile (64, 64): one ``EventPlan.contrast_dense_hvp`` without and with
a reused ``state``, against what a gradient costs on the same full plan and against eager torch double backward of the restated
expression on the same GPU -- one process, the legs alternating, best of ``--rounds`` rounds, warmed up, a device synchronise inside
the clock:

    (a) hessp        contrast_dense_hvp(flow, v): tangent + IWE windows, two cost passes, the owner kernel (value, d_flow, hv)
    (b) hessp_state  contrast_dense_hvp(flow, v, state=...): the tangent window alone, one cost pass, the owner kernel (hv)
    (c) gradient     one forward + backward of contrast_dense on the same plan: the price of a gradient before this operator
    (d) torch        the variance of the bilinear IWE written in torch ops, float32, hv by double backward

    python tools/bench_hvp.py [--out profiles/hvp_bench.json] [--rounds 5] [--reps 20]
    python tools/bench_hvp.py --solver                      # + tools/run_cmax.py's synthetic window: Newton-CG against L-BFGS-B
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_hvp.py --kernels --case 0   # a run of its own per case: the products alone
    python tools/bench_hvp.py --kernel-stats 0=DIR/.../*_kernel_stats.csv,1=...              # ... the kernels' times against the algorithmic bytes

Reports each best and its max - min spread over the rounds; a difference counts only where the intervals [best, best + spread] lie
apart.  Prints one JSON document."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_bos_amd as ebos  # noqa: E402

CASES = [("2M@1280x720", 2_000_000, (720, 1280)), ("100k@346x260", 100_000, (260, 346))]
TILE = (64, 64)
KERNELS = ("iwe_tangent_tiled_kernel", "iwe_tangent_combine_kernel", "iwe_hvp_owner_bwd_kernel")


def synth(n, shape, seed=0):
    """Sub-pixel source coordinates (off the kinks of the vote at any flow, almost surely), times sorted on [0, 1]; a smooth flow of a
    few pixels (BOS displacements are small) and a smooth direction of the same kind."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    H, W = shape
    ev = torch.stack([torch.rand(n, generator=g, dtype=torch.float64) * (H - 1e-3), torch.rand(n, generator=g, dtype=torch.float64) * (W - 1e-3),
                      torch.sort(torch.rand(n, generator=g, dtype=torch.float64)).values, torch.randint(0, 2, (n,), generator=g).double()], 1)
    ev[0, 2], ev[-1, 2] = 0.0, 1.0
    smooth = lambda amp: torch.nn.functional.interpolate((torch.rand((1, 2, 6, 8), generator=g) * 2 - 1) * amp, size=shape,   # noqa: E731
                                                         mode="bicubic", align_corners=False)[0].contiguous()
    return ev.cuda(), smooth(3.0).cuda(), smooth(1.0).cuda()


def torch_variance(plan, flow):
    """var(IWE(flow)) of the plan's events in torch ops (float32, scatter-add), twice differentiable in the flow."""
    H, W = plan.image_size
    x, y, dt = plan.x, plan.y, plan.dt
    lin = x.long() * W + y.long()
    xw, yw = x - dt * flow[0].reshape(-1)[lin], y - dt * flow[1].reshape(-1)[lin]
    r0, c0 = torch.floor(xw + 1e-6), torch.floor(yw + 1e-6)
    fr, fc = xw - r0, yw - c0
    R, C = r0.long(), c0.long()
    img = torch.zeros(H * W, dtype=flow.dtype, device=flow.device)
    for dr, dc, wgt in ((0, 0, (1 - fr) * (1 - fc)), (1, 0, fr * (1 - fc)), (0, 1, (1 - fr) * fc), (1, 1, fr * fc)):
        ok = (R + dr >= 0) & (R + dr < H) & (C + dc >= 0) & (C + dc < W)
        img = img.index_add(0, torch.where(ok, (R + dr) * W + C + dc, torch.zeros_like(R)), wgt * ok)
    return img.var()


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def measure(legs, rounds):
    for fn, _ in legs.values():   # warm-up: code objects, workspaces, jobs, allocator pools
        for _ in range(3):
            fn()
    samples = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, reps) in legs.items():
            samples[k].append(timed(fn, reps))
    return {k: {"best_us": round(min(v), 2), "spread_us": round(max(v) - min(v), 2), "rounds_us": [round(x, 2) for x in v]}
            for k, v in samples.items()}


def algorithmic_bytes(n, shape, with_iwe, with_grad, halo=16):
    """What the kernels must move at the least (events once, every slab and image cell once per read or write), from the shapes alone;
    float64 slabs."""
    H, W = shape
    tiles = -(-H // TILE[0]) * -(-W // TILE[1])
    n_keys = tiles * TILE[0] * TILE[1]
    slabs = tiles * (2 if with_iwe else 1) * (TILE[0] + 2 * halo) * (TILE[1] + 2 * halo) * 8
    tangent = 12 * n + 2 * 8 * H * W + slabs                                       # x, y, dt; flow and v; the tiles' windows stored
    combine = slabs + (2 if with_iwe else 1) * 8 * H * W                           # the slabs read; read-modify-write of the image(s)
    owner = 12 * n + 4 * (n_keys + 1) + 2 * 8 * H * W + 2 * 4 * H * W + (2 if with_grad else 1) * 8 * H * W   # + offsets, G1 and G2, hv (+ d_flow)
    return {"tangent": tangent, "combine": combine, "owner": owner}


def run_case(name, n, shape, rounds, reps):
    ev, flow, v = synth(n, shape)
    plan = ebos.EventPlan.build(ev, shape, "first", True, tile=TILE, emit="full")
    leaf = flow.clone().requires_grad_(True)
    _, _, hv, state = plan.contrast_dense_hvp(flow, v)

    def gradient():
        leaf.grad = None
        plan.contrast_dense(leaf).backward()
        return leaf.grad

    def torch_hvp():
        f = flow.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(torch_variance(plan, f), f, create_graph=True)
        return torch.autograd.grad((g * v).sum(), f)[0]

    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    agree = {"hv_vs_torch_double_backward": rel(hv, torch_hvp()), "hv_state_vs_no_state": rel(plan.contrast_dense_hvp(flow, v, state=state)[2], hv),
             "d_flow_vs_contrast_dense": rel(state["d_flow"], gradient())}
    legs = {"hessp": (lambda: plan.contrast_dense_hvp(flow, v), reps),
            "hessp_state": (lambda: plan.contrast_dense_hvp(flow, v, state=state), reps),
            "gradient": (gradient, reps), "torch": (torch_hvp, max(1, reps // 5))}
    lib = ebos.load_library()
    res = {"case": name, "events": n, "image": list(shape), "tile": list(TILE), "halo": state["halo"],
           "windows": {"with_iwe": {2: "f64", 1: "f32"}[int(lib.ebos_iwe_multiref_fits(TILE[0], TILE[1], state["halo"], 2))],
                       "tangent_alone": {2: "f64", 1: "f32"}[int(lib.ebos_iwe_multiref_fits(TILE[0], TILE[1], state["halo"], 1))]},
           "agreement": agree, "legs": measure(legs, rounds),
           "algorithmic_bytes": {"hessp": algorithmic_bytes(n, shape, True, True), "hessp_state": algorithmic_bytes(n, shape, False, False)}}
    plan.clear_cache()
    return res


def run_kernels(cases, calls=20):
    """The launches a profiler should see: ``calls`` products without and with a state per case (the tangent kernel with and without
    the IWE window, the owner kernel with and without d_flow).  A profiler's statistics sum by kernel name: one case per run."""
    for name, n, shape in cases:
        ev, flow, v = synth(n, shape)
        plan = ebos.EventPlan.build(ev, shape, "first", True, tile=TILE, emit="full")
        state = None
        for _ in range(calls):
            state = plan.contrast_dense_hvp(flow, v)[3]
        for _ in range(calls):
            plan.contrast_dense_hvp(flow, v, state=state)
        torch.cuda.synchronize()


def kernel_stats(spec):
    """``CASE=CSV[,CASE=CSV]``: per-kernel times of rocprofv3 ``--stats`` CSVs of ``--kernels --case CASE`` runs, for the two new
    kernels, with the algorithmic bytes of the case and the rate they imply at the mean time.  The statistics sum by kernel name: the
    template arguments tell the tangent kernel's two forms apart (``Lb1``: with the IWE window), the owner kernel reports one row
    for its calls with and without d_flow, the combine kernel one row for one and two images (the bytes given are those with d_flow
    and with two images)."""
    out = []
    for item in spec.split(","):
        case, path = item.split("=", 1)
        name_of_case, n, shape = CASES[int(case)]
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            if not any(k in name for k in KERNELS):
                continue
            with_iwe = "double, true," in name or "float, true," in name
            which = "tangent" if KERNELS[0] in name else ("combine" if KERNELS[1] in name else "owner")
            nbytes = algorithmic_bytes(n, shape, with_iwe or which == "combine", True)[which]
            mean_us = float(r["AverageNs"]) / 1e3
            out.append({"case": name_of_case, "kernel": name, "calls": int(r["Calls"]), "mean_us": round(mean_us, 2),
                        "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2),
                        "algorithmic_bytes": nbytes, "GB_per_s_at_mean": round(nbytes / mean_us / 1e3, 1)})
    return out


def run_solver():
    """tools/run_cmax.py's synthetic window through configs/cmax_newton_cg.yaml, and through the same file with L-BFGS-B."""
    import yaml

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_cmax

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cmax_newton_cg.yaml")))
    events, shape = run_cmax.synthetic_window(cfg)
    truth = run_cmax.dense_truth(cfg["data"])
    out = []
    for method in ("Newton-CG", "trust-ncg", "trust-krylov", "L-BFGS-B"):
        scfg = json.loads(json.dumps(cfg["solver"]))
        scfg["optimizer"]["method"] = method
        if method != "Newton-CG":
            scfg["optimizer"].pop("options", None)
        slv = ebos.solver.ContrastMaximization(shape, shape, solver_config=scfg)
        slv.estimate(events)   # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flow = slv.estimate(events)
        wall = time.perf_counter() - t0
        epe = float(np.sqrt(((flow - truth) ** 2).sum(0)).mean())
        out.append({"method": method, "loop_mode": slv.loop_mode, "fused": bool(slv.fused), "evaluations": len(slv.history),
                    "products": int(slv.hessp_calls), "scipy_iterations": int(slv.scipy_result.nit), "wall_ms": round(wall * 1e3, 2),
                    "loss_first": slv.history[0], "loss_final": float(slv.scipy_result.fun), "epe_px": round(epe, 4),
                    "epe_zero_flow_px": round(float(np.sqrt((truth ** 2).sum(0)).mean()), 4), "message": str(slv.scipy_result.message)})
    return {"window": {"events": int(len(events)), "image": list(shape), "config": "configs/cmax_newton_cg.yaml"}, "runs": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--solver", action="store_true", help="also run the end-to-end comparison on run_cmax.py's synthetic window")
    ap.add_argument("--kernels", action="store_true", help="only launch the products (for a profiler's run)")
    ap.add_argument("--case", type=int, default=None, help="with --kernels: the index of the one case to launch (0: 2 M events, 1: 100 k)")
    ap.add_argument("--kernel-stats", default=None, metavar="CASE=CSV,...",
                    help="rocprofv3 --stats kernel CSVs of --kernels --case runs, merged into the report")
    args = ap.parse_args()
    ebos.load_library()
    if args.kernels:
        run_kernels(CASES if args.case is None else [CASES[args.case]])
        return
    doc = {"tool": "tools/bench_hvp.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
           "unit": "microseconds per call, device synchronise inside the clock",
           "notes": "agreement.hv_vs_torch_double_backward is recorded, not judged: the torch leg floors absolute float32 coordinates "
                    "(1e-4 px at 1280 px), so events near a kink of the vote land on its other side; what the kernels keep of the float64 "
                    "product is bounded in tests/test_gpu_hvp.py",
           "results": [run_case(name, n, shape, args.rounds, args.reps) for name, n, shape in CASES]}
    doc["kernels"] = kernel_stats(args.kernel_stats) if args.kernel_stats else "not measured"
    doc["solver"] = run_solver() if args.solver else "not measured"
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
