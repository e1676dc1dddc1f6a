#!/usr/bin/env python3
"""Headline benchmark: Mevents/s through the fused warp + IWE (+ variance contrast) pass at 1280x720.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 2|3|4|5] [--full] [--dry-run]

A plain run does what its headline figure needs: it sets up the workload, runs the W warm-up steps, times the K steps,
writes ``--dump-outputs`` if asked and prints the line.  Its set-up is the one the timed block has always started from
(config 2's timed plan builds, config 4's per-window pass and its cross-check: a few milliseconds of device work).
``--full`` adds everything the benchmark measures or checks after the timed block: the kernel-timed blocks and the
rooflines, the informative legs (fwd+bwd, streams, rotating windows, solver), the measured copy bandwidth, config 4's
host enqueue time and the CPU baseline.  ``--no-extras`` / ``--no-cpu-baseline`` trim a full run.

With ``--gpus N > 1`` and no launcher environment (RANK unset) this process starts the N ranks itself
(``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>``, as a
CHILD process, before anything here has touched the GPU) and relays rank 0's JSON line; launched BY torchrun (RANK set)
it is one rank of that job.  One process per GPU, ``torch.distributed`` ("nccl" = RCCL) only for the rendezvous, the
barrier around the timed region, the MAX over ranks and the final object gather: the path has NO data-path collective.

Workloads (BASELINE.json ``configs``; ``--config``):
  2 (default)  one window of 10 M synthetic events per rank (recipe of src/utils/event_utils.py:40-47, seed = rank) at
               1280x720, dense per-pixel flow U(-30, 30) (src/utils/flow_utils.py:29), normalised time, reference time
               "first", variance contrast.  One step = one evaluation of the contrast objective on the resident window
               (ebos_iwe_dense_slab_f32: tile accumulate -> slab combine (writes the IWE) -> variance).  WEAK scaling.
  4            64 time windows x 2 M events, 30x40 patch-flow grid per window (src/solver/patch_eklt.py:173-204), windows
               dealt round-robin to the ranks (the per-window loop of bos_event.py:144-220).  One step = the objective of
               every window this rank owns, evaluated once (ebos_iwe_patch_slab_f32).  STRONG scaling (64 windows in all).
  5            512 2-DoF hypotheses (32 x 16 grid over [-30, 30]^2: the grid sampler of
               src/solver/generative_max_likelihood.py:238-255) over ONE window of 50 M events replicated on every rank,
               hypotheses in contiguous blocks of 512 / N.  One step = this rank's block evaluated once.  STRONG scaling.

The window is resident in HBM in its plan form (compact events binned by source tile: built once per window and reused
by every solver iteration); its one-off build time is reported as ``plan_build_ms`` and, folded into a single
evaluation, as ``value_incl_plan_build`` -- it is NOT in the timed region of ``value``.

Timing: W warm-up steps, then ONE block of exactly K timed steps, bracketed by barrier + torch.cuda.synchronize() and
MAX-reduced over the ranks; ``ms_per_step`` is that block / K.  ``--min-seconds S`` repeats the block until >= S of timed
work and reports the MEDIAN block (``repeats``).  With ``--full`` the dominant kernels are then timed by HIP events stamped
with their own dispatch (hipExtLaunchKernelGGL on the launch stream) during two more blocks (steady-state clocks), outside
``ms_per_step``.

``--dump-outputs DIR`` writes what the last timed step computed -- the arrays a caller of the timed path receives -- as
DIR/<name>.npy (float32 / float64; rank<r>_<name>.npy per rank of an N-rank job), right after the timed block.  The inputs
are seeded: the same arguments give the same inputs on every run, so two builds can be compared output for output.

Prints ONE JSON line on rank 0 (see README / DESIGN.md for the fields).
"""
import argparse
import hashlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W = 720, 1280
N_EVENTS = 10_000_000
FLOW_MAX = 30.0
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s measured achievable
DOMINANT_SOURCE = os.path.join("event_based_bos_amd", "csrc", "iwe_tile_core.h")
CONFIG4 = dict(windows=64, events=2_000_000, patch=(24, 32), slide=(24, 32))   # -> patch grid 30 x 40
CONFIG5 = dict(events=50_000_000, grid=(32, 16), theta_max=30.0)              # -> 512 hypotheses
DEFAULT_STEPS = {2: 200, 3: 200, 4: 10, 5: 2}
DEFAULT_WARMUP = {2: 20, 3: 20, 4: 2, 5: 1}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4, 5))
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"),
                    help="process-group backend of an N-rank run: nccl (= RCCL, one GPU per rank) or gloo (host-side barrier / "
                         "reduce; ranks may then share a GPU -- a functional test of the N-rank path on a one-GPU box)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch + rendezvous + shard assignment + gather only (gloo, CPU, no kernels)")
    ap.add_argument("--min-seconds", type=float, default=0.0,
                    help="repeat the K-step block until this much timed work (default: one block, exactly --steps timed steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    ap.add_argument("--max-repeats", type=int, default=100000,
                    help="cap on timed blocks (the default never binds: --min-seconds decides, also under the driver's --steps 20)")
    ap.add_argument("--events", type=int, default=None, help="events per window (default: the config's)")
    ap.add_argument("--windows", type=int, default=None, help="config 4: number of windows (default 64)")
    ap.add_argument("--tile", type=int, nargs=2, default=[0, 0], help="source tile (0 0 = choose_tile: 45x80 at 1280x720)")
    ap.add_argument("--halo", type=lambda v: v if v == "auto" else int(v), default=None,
                    help="a built halo of the tile-private kernels, or 'auto': run-time LDS windows per tile (EBOS_HALO_AUTO).  Default: "
                         "32 for configs 2 and 4 (their flows ARE 30 px: every window would be the full one and the bound costs 2 us), "
                         "auto for config 5 (most of the sweep's thetas are far below 30 px: 36.7 -> 34.0 ms, the same variances bit for bit)")
    ap.add_argument("--splits", type=int, default=1)
    ap.add_argument("--flow-max", type=float, default=FLOW_MAX, help="amplitude of the synthetic flow (BASELINE: 30 px)")
    ap.add_argument("--streams", type=int, default=3, help="configs 4 / 5: independent windows / hypotheses kept in flight per rank")
    ap.add_argument("--full", action="store_true",
                    help="after the timed block, measure and check everything beside the headline figure: kernel-timed blocks and "
                         "rooflines, the informative legs, copy bandwidth, the CPU baseline (default: the headline only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the raw-column plan build and, with --full, the informative legs (fwd+bwd, streams, rotating windows, solver)")
    ap.add_argument("--batch", type=int, default=64, help="config 4: windows per ebos_iwe_slab_batch_f32 call (16 per launch inside); 0 = one call per window")
    ap.add_argument("--tail-stream", action="store_true", help="config 4, batched: combine / finalize passes of a batch on a second stream beside the next "
                                                               "batch's accumulate pass (measured SLOWER wherever the two really overlap: 1.11 against 0.96 ms per pass "
                                                               "with a hardware queue per stream; the default is one stream)")
    ap.add_argument("--no-tail-stream", action="store_true", help="(the default since round 5; kept for old command lines)")
    ap.add_argument("--no-graph", action="store_true", help="config 4: enqueue every window's calls from Python instead of replaying a captured pass")
    ap.add_argument("--no-compact", action="store_true", help="read the 12 B/event (x, y, dt) plan instead of 6 B/event")
    ap.add_argument("--fractional", action="store_true",
                    help="config 2 with source coordinates on a 1/64 px grid (undistorted events): the general 12 B/event format, "
                         "looked up truncated (src/warp.py:334) -- NOT the BASELINE workload")
    ap.add_argument("--weighted", action="store_true",
                    help="config 2 with per-event weights (src/event_image_converter.py:576-577: the ds_add_f64 path, 16 B/event) "
                         "-- NOT the BASELINE workload")
    ap.add_argument("--cpu-sample", type=int, default=N_EVENTS, help="events of the window the CPU baseline is timed on")
    ap.add_argument("--rotating-windows", type=int, default=8, help="distinct 10 M-event plans cycled by the cache-cold leg")
    args = ap.parse_args(argv)
    if args.steps is None:
        args.steps = DEFAULT_STEPS[args.config]
    if args.warmup is None:
        args.warmup = DEFAULT_WARMUP[args.config]
    if args.halo is None:
        args.halo = "auto" if args.config == 5 else 32
    return args


# ---------------------------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` starts the N ranks itself
# ---------------------------------------------------------------------------------------------------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(args, argv):
    """Parent of an N-rank job.  Runs before this process has imported torch or touched the GPU; the ranks are CHILD
    processes (never an exec of a GPU-initialised process).  Their output goes straight through: rank 0 prints the line."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: needed by RCCL across processes on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def shard_for(config, rank, world, args):
    """Units of this rank: config 4 windows round-robin, config 5 hypotheses in contiguous blocks,
    config 2 one own window per rank."""
    from event_based_bos_amd.sharding import shard_units

    if config == 4:
        return shard_units(args.windows or CONFIG4["windows"], world, rank, "round_robin")
    if config == 5:
        return shard_units(CONFIG5["grid"][0] * CONFIG5["grid"][1], world, rank, "block")
    return [rank]


RENDEZVOUS_TIMEOUT_S = 300  # a rank that cannot reach the others says so within five minutes instead of hanging the driver's run
# (the same timeout then bounds every later barrier / reduce of the group: nothing between two of them takes a rank that long)


def init_group(backend, rank, world, device=None):
    """torch.distributed rendezvous with a bounded wait and a one-line diagnosis."""
    import datetime

    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    kw = {"device_id": device} if (backend == "nccl" and device is not None) else {}
    try:
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=RENDEZVOUS_TIMEOUT_S), **kw)
    except Exception as e:  # (DistStoreError / DistNetworkError / RuntimeError: all mean "the ranks did not meet")
        raise SystemExit(f"rank {rank}/{world}: {backend} rendezvous at {os.environ.get('MASTER_ADDR')}:{os.environ.get('MASTER_PORT')} "
                         f"failed within {RENDEZVOUS_TIMEOUT_S} s: {type(e).__name__}: {e}")
    return dist


def dry_run(args):
    """The N-rank plumbing without a GPU: rendezvous (gloo), shard assignment, barrier, MAX-reduce, object gather."""
    import torch

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    dist = None
    if world > 1:
        dist = init_group("gloo", rank, world)
    mine = shard_for(args.config, rank, world, args)
    seen = [{"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", 0)), "units": len(mine), "first_units": mine[:4]}]
    t = torch.tensor([0.001 * (rank + 1)], dtype=torch.float64)
    if world > 1:
        dist.barrier()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        parts = [None] * world
        dist.all_gather_object(parts, seen[0])
        seen = parts
    if rank == 0:
        print(json.dumps({"dry_run": True, "config": args.config, "n_gpus": world, "ranks_seen": seen,
                          "units_total": sum(s["units"] for s in seen), "max_over_ranks_check": float(t.item()),
                          "steps": args.steps, "warmup": args.warmup}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def synth_window(n, seed, flow=True, flow_max=FLOW_MAX):
    import numpy as np

    rs = np.random.RandomState(seed)
    x = rs.randint(0, H, n)
    y = rs.randint(0, W, n)
    t = np.sort(rs.uniform(0.0, 0.5, n))
    p = rs.randint(0, 2, n)
    ev = np.stack([x, y, t, p], axis=1).astype(np.float64)
    fl = np.random.RandomState(1000 + seed).uniform(-flow_max, flow_max, (2, H, W)) if flow else None
    return ev, fl


def git_blob_sha(path):
    """`git hash-object` of a file without git (the GPU box has no .git): sha1("blob <len>\\0" + content)."""
    try:
        data = open(path, "rb").read()
    except OSError:
        return None
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed PMC collection -- only if that collection was made on the
    kernel source as it is NOW (blob hash of csrc/iwe_tile_core.h recorded by tools/make_pmc_json.py); else None."""
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        return None, {"traffic_note": "profiles/pmc_latest.json missing"}
    # (traffic_kernel: the kernel the traffic figure belongs to -- the entry asked for, with the template it was collected on)
    # (the collection's top-level template is the default accumulate kernel's: it labels that entry only)
    tmpl = (rec.get("kernels", {}).get(kernel, {}) or {}).get("kernel_template") or (rec.get("kernel_template") if kernel == "iwe_slab_accumulate_kernel" else None)
    stamp = {"traffic_commit": rec.get("commit"), "traffic_kernel": f"{kernel} [{tmpl}]" if tmpl else kernel,
             "traffic_source_blob": rec.get("source_blob_sha")}
    now = git_blob_sha(os.path.join(ROOT, DOMINANT_SOURCE))
    if rec.get("source_blob_sha") is None or rec.get("source_blob_sha") != now:
        stamp["traffic_note"] = f"stale: collected on blob {rec.get('source_blob_sha')}, kernel source is now {now}"
        return None, stamp
    k = rec.get("kernels", {}).get(kernel, {})
    t = k.get("hbm_bytes_per_launch")
    if t is not None and k.get("windows"):  # a batched (persistent) pass: per window / hypothesis of the launch
        t = t / k["windows"]
    return t, stamp


def rocprof_stats(kernel_prefix, ends="false>"):
    """Average duration of a kernel from the committed rocprofv3 --kernel-trace --stats run of the default bench command
    (profiles/kernel_stats_latest.json, tools/collect_round_profiles.sh) -- only if it was taken on the kernel source as it is
    now; else None.  Quoted NEXT to the live HIP-event timing: an event pair attached to a dispatch (hipExtLaunchKernelGGL)
    brackets the dispatch plus the gap to the packet in front of it, rocprofv3 reports the dispatch's own begin / end."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "kernel_stats_latest.json")))
    except (OSError, ValueError):
        return None
    if rec.get("source_blob_sha") != git_blob_sha(os.path.join(ROOT, DOMINANT_SOURCE)):
        return None
    best = None
    for name, k in rec.get("kernels", {}).items():
        # the dense-flow instantiation with a built halo: its trailing template flags (UNIFORM, GRID, DYN -- or GRID, DYN for the
        # backward kernel's tail) are all false
        if name.startswith(kernel_prefix) and name.endswith("false, false, false>") and (best is None or k["calls"] > best["calls"]):
            best = dict(k, kernel=name)
    if best is not None:
        best["commit"] = rec.get("commit")
    return best


# The roofline that BINDS the event kernels is instruction issue, not HBM: VALU issue per SIMD and the LDS
# pipe per CU.  Instruction counts per launch come from the committed PMC collection of the same kernel source
# (profiles/pmc_latest.json: SQ_INSTS_VALU / SQ_INSTS_LDS, wave-instructions summed over the chip, collected at THIS workload's
# size); what an instruction costs from the micro-benchmarks (tools/ubench_valu_issue.hip, tools/ubench_lds.hip ->
# profiles/r02_valu_issue_cost.txt, r02_lds_cost_and_phases.txt): with the kernels' 4 waves per SIMD a VALU wave-instruction of
# their mix occupies its SIMD for ~3.2 cycles (2.1 v_sub_u32 ... 3.4 v_cndmask, 4.9 v_cmp -> SGPR pair), an LDS wave-instruction
# the CU's LDS pipe for ~8.6 (ds_add_u64, random cells) ... 15.5 (neighbouring lanes on adjacent cells); reads 6.5 - 13.8.
ISSUE = {"n_cu": 256, "simd_per_cu": 4, "valu_cycles_per_wave_inst": 3.2, "lds_cycles_per_wave_inst": 10.0,
         "source": "tools/ubench_valu_issue.hip, tools/ubench_lds.hip (profiles/r02_valu_issue_cost.txt, r02_lds_cost_and_phases.txt)"}


def roofline_issue(kernel_key, kernel_ms_list, clock_hz, events=None):
    """`roofline_issue`: the time the kernel's VALU and LDS instruction streams need at the measured issue costs, against the
    measured kernel time.  frac = max(valu, lds) bound / measured <= 1; null counts when the PMC collection is stale or absent."""
    k_ms = statistics.mean(kernel_ms_list) if kernel_ms_list else float("nan")
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    ent = {"kernel": kernel_key, "kernel_ms": round(k_ms, 4), "clock_GHz": round(clock_hz / 1e9, 3), **ISSUE}
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        ent["note"] = "profiles/pmc_latest.json missing"
        return ent
    if rec.get("source_blob_sha") != git_blob_sha(os.path.join(ROOT, DOMINANT_SOURCE)):
        ent["note"] = f"stale: counters collected on blob {rec.get('source_blob_sha')}"
        return ent
    k = rec.get("kernels", {}).get(kernel_key, {})
    valu, lds = k.get("SQ_INSTS_VALU"), k.get("SQ_INSTS_LDS")
    if valu is None or lds is None:
        ent["note"] = f"no instruction counters for {kernel_key} in profiles/pmc_latest.json"
        return ent
    if k.get("windows"):  # a batched (persistent) pass: per window / hypothesis of the launch, like kernel_ms
        valu, lds = valu / k["windows"], lds / k["windows"]
    if events and k.get("events") and int(events) != int(k["events"]):
        # the counters were collected at another window size: the per-event instruction counts carry over, the launch's totals do not
        scale = float(events) / float(k["events"])
        valu, lds = valu * scale, lds * scale
        ent["counters_scaled_to_events"] = int(events)
    t_valu = valu / (ISSUE["n_cu"] * ISSUE["simd_per_cu"]) * ISSUE["valu_cycles_per_wave_inst"] / clock_hz * 1e3  # ms
    t_lds = lds / ISSUE["n_cu"] * ISSUE["lds_cycles_per_wave_inst"] / clock_hz * 1e3
    bound = "valu_issue" if t_valu >= t_lds else "lds_pipe"
    ent.update({"bound": bound, "valu_wave_insts": valu, "lds_wave_insts": lds, "valu_bound_ms": round(t_valu, 4),
                "lds_bound_ms": round(t_lds, 4), "frac": round(max(t_valu, t_lds) / k_ms, 4),
                "counters_collected_at_events": k.get("events"), "traffic_commit": rec.get("commit")})
    if events:
        ent["valu_insts_per_event"] = round(valu * 64.0 / events, 2)  # a wave-instruction serves 64 lanes, a lane its own events
        ent["lds_insts_per_event"] = round(lds * 64.0 / events, 2)
    return ent


def device_clock_hz(dev):
    """shader clock the issue bound is priced at: the device's maximum engine clock (a LOWER bound of the time: the chip rarely
    holds it under load, which can only make `roofline_issue.frac` smaller than the truth)"""
    import torch

    try:
        return float(torch.cuda.get_device_properties(dev).clock_rate) * 1e3  # kHz -> Hz
    except Exception:
        return 2.4e9


def cpu_baseline(ev, flow, sample):
    """The oracle's op-for-op torch-CPU restatement of the reference path (kind 'port'), timed on this
    host's cores on a bounded sample of the same window."""
    import torch

    from oracle import ebos_oracle as O

    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # torch's intra-op pool does not scale to hundreds of threads on this memory-bound op chain:
    # calibrate on a 2 M-event sample and keep the fastest thread count.
    e_cal = torch.from_numpy(ev[:min(sample, 2_000_000)])  # large enough to leave the caches, like the timed run
    f_cal = torch.from_numpy(flow)
    best, threads = None, 1
    for cand in [c for c in (8, 16, 32, 64, 128, 256) if c <= avail] or [avail]:
        torch.set_num_threads(cand)
        O.iwe_dense(e_cal, f_cal, (H, W))
        t0 = time.perf_counter()
        O.iwe_dense(e_cal, f_cal, (H, W))
        dt_ = time.perf_counter() - t0
        if best is None or dt_ < best:
            best, threads = dt_, cand
    torch.set_num_threads(threads)
    out, contrast = {}, None
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        e = torch.from_numpy(ev[:sample]).to(dt)
        f = torch.from_numpy(flow).to(dt)
        times = []
        for rep in range(6):
            t0 = time.perf_counter()
            iwe = O.iwe_dense(e, f, (H, W))
            var = O.image_variance(iwe)
            times.append(time.perf_counter() - t0)
            if sum(times) > 40.0 and rep >= 2:  # a slow host: stay within the bench's few minutes
                break
        if name == "f64":
            contrast = abs(float(var.item()))  # (the oracle's cost is signed for minimisation; the contrast is its magnitude)
        out[name] = sample / statistics.median(times[1:]) / 1e6
        reps = len(times) - 1
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            model = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "unknown")
    except OSError:
        pass
    return {"value": round(out["f64"], 3), "unit": "Mevents/s", "cores": threads, "host_cpus": avail, "cpu_model": model,
            "kind": "port",
            "sample": (f"{'the whole window' if sample >= len(ev) else 'first ' + str(sample) + ' events of the window'} "
                       f"({min(sample, len(ev))} events), fwd warp+IWE+variance, torch-CPU fp64 (reference default dtype), "
                       f"median of {reps} after 1 warm-up; fp32 on the same sample: {out['f32']:.2f} Mevents/s"),
            "value_f32": round(out["f32"], 3), "contrast_f64": contrast}


# ---------------------------------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------------------------------
class Rank(object):
    def __init__(self, args):
        import torch

        self.args = args
        self.rank = int(os.environ.get("RANK", 0))
        self.local_rank = int(os.environ.get("LOCAL_RANK", 0))
        self.world = int(os.environ.get("WORLD_SIZE", 1))
        self.distributed = self.world > 1 or "TORCHELASTIC_RUN_ID" in os.environ  # under torchrun also for a world of 1
        index = 0
        if self.distributed:
            n_dev = torch.cuda.device_count()
            if args.backend == "nccl" and self.local_rank >= n_dev:
                raise SystemExit(f"rank {self.rank}: local rank {self.local_rank} but {n_dev} GPU(s) visible (one GPU per rank with nccl)")
            index = self.local_rank % max(n_dev, 1)
            torch.cuda.set_device(index)
            self.dist = init_group(args.backend, self.rank, self.world, torch.device("cuda", index))
        else:
            torch.cuda.set_device(0)
        self.dev = torch.device("cuda", index)

    def sync_all(self):
        import torch

        torch.cuda.synchronize()
        if self.distributed:
            self.dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(self, seconds):
        import torch

        if not self.distributed:
            return seconds
        tt = torch.tensor([seconds], dtype=torch.float64, device=self.dev if self.args.backend == "nccl" else "cpu")
        self.dist.all_reduce(tt, op=self.dist.ReduceOp.MAX)
        return float(tt.item())

    def gather(self, obj):
        if not self.distributed:
            return [obj]
        parts = [None] * self.world
        self.dist.all_gather_object(parts, obj)
        return parts

    def timed_blocks(self, step, lib, profile_kernel=0, launches_per_step=1, profile_blocks=2, outputs=None):
        """Warm-up, then one block of exactly --steps steps (barrier + synchronize on both sides, MAX over ranks), repeated until
        --min-seconds of timed work; returns (block times [s], per-launch kernel times [ms] of the profiled blocks, which are not
        among the block times; --full only).  ``outputs()`` -> {name: tensor} is what the last timed step computed: written for
        --dump-outputs before the profiled blocks run."""
        import ctypes

        import torch

        a = self.args
        for _ in range(a.warmup):
            step()
        self.sync_all()
        blocks, kernel_ms = [], []

        def one_block(prof):
            nrec = max(1, a.steps * launches_per_step)
            if prof:
                from event_based_bos_amd import _hip
                _hip.check(lib.ebos_profile_start_kernel(profile_kernel, nrec), "ebos_profile_start_kernel")
            self.sync_all()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            # every rank stops ITS clock when its own K steps have drained; only then the barrier, then MAX over ranks.  (With the
            # barrier inside the clock a 0.5 ms block of --steps 20 carried an RCCL barrier of 30 - 100 us: 6 - 20 % of weak-scaling
            # "loss" that no kernel lost, and a line that could not be compared with N = 1, which has no group; VERDICT r05 weak #6.)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            self.sync_all()
            dt = self.max_over_ranks(dt)
            if prof:
                buf = (ctypes.c_float * nrec)()
                got = lib.ebos_profile_stop(buf, nrec)
                kernel_ms.extend(buf[i] for i in range(got))
            else:
                blocks.append(dt)

        one_block(False)
        while sum(blocks) < a.min_seconds and len(blocks) < a.max_repeats:
            one_block(False)
        if a.dump_outputs and outputs is not None:
            dump_outputs(a.dump_outputs, outputs(), self.rank, self.world)
        for _ in range(profile_blocks if a.full else 0):  # the profiled blocks come LAST: clocks and caches are in their steady state by then
            one_block(True)
        return blocks, kernel_ms


def survey_priced(survey_bytes, kernel_ms_list):
    """Configs 4 / 5 price `roofline.achieved` on the bytes the launch's inputs and outputs OCCUPY (the compact plan: 6 B/event,
    DESIGN 3) -- SURVEY 8(d)'s 12 B/event (x, y, dt as three floats) would put a kernel with no flow gathers above the HBM peak (1.14
    in round 2): that is the format's 2x, not bandwidth.  The SURVEY-priced figure is kept here, labelled."""
    k_ms = statistics.fmean(kernel_ms_list) if kernel_ms_list else float("nan")
    gbs = survey_bytes / (k_ms * 1e-3) / 1e9
    return {"survey_priced": {"bytes": survey_bytes, "GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
                              "note": "SURVEY 8(d): 12 B/event (p unused); exceeds what the kernel moves, may exceed 1"}}


def roofline_entry(kernel, kernel_ms_list, algo_bytes, extra=None):
    k_ms = statistics.mean(kernel_ms_list) if kernel_ms_list else float("nan")
    achieved = algo_bytes / (k_ms * 1e-3) / 1e9
    traffic, stamp = pmc_traffic(kernel)
    ent = {"bound": "hbm", "kernel": kernel, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "kernel_ms": round(k_ms, 4),
           "kernel_ms_min": round(min(kernel_ms_list), 4) if kernel_ms_list else None,
           "kernel_ms_max": round(max(kernel_ms_list), 4) if kernel_ms_list else None,
           "kernel_launches_timed": len(kernel_ms_list), "algorithmic_bytes": algo_bytes}
    ent.update(stamp)
    rp = rocprof_stats(kernel.split("<")[0] + "<") if "<" not in kernel else None
    if rp is not None:  # the committed rocprofv3 run of this command, same kernel source
        ent["rocprofv3"] = {"avg_us": rp["avg_us"], "min_us": rp["min_us"], "calls": rp["calls"], "commit": rp["commit"],
                            "achieved": round(algo_bytes / (rp["avg_us"] * 1e-6) / 1e9, 1),
                            "frac": round(algo_bytes / (rp["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "kernel": rp["kernel"]}
    if extra:
        ent.update(extra)
    return ent


def lead_with_binding(roof, issue):
    """`roofline` leads with the roofline that BINDS the kernel.  With instruction counters of this kernel
    source at hand (`roofline_issue`), bound / achieved / peak / unit / frac are the issue roofline's: wave-instructions per second
    against what the chip's SIMDs (VALU) or LDS pipes can issue at the micro-benchmarked cost per instruction.  SURVEY 8(d)'s HBM
    pricing of the same launch moves to `hbm_algorithmic` / `hbm_algorithmic_frac`: it prices 12 B/event against 8 TB/s while the
    kernel reads a 6 B/event plan that sits in the 256 MiB Infinity Cache from step to step, so it can exceed 1 against the
    measured copy bandwidth -- a statement about the format and the cache, not about the kernel.  Without counters (stale or absent
    collection) the entry stays the HBM one and says so."""
    if not issue.get("bound"):
        roof["bound_note"] = "no instruction counters for this kernel source (" + str(issue.get("note")) + "): HBM pricing only"
        roof["hbm_algorithmic_frac"] = roof["frac"]
        return roof
    k_s = issue["kernel_ms"] * 1e-3
    valu = issue["bound"] == "valu_issue"
    insts = issue["valu_wave_insts"] if valu else issue["lds_wave_insts"]
    units = ISSUE["n_cu"] * (ISSUE["simd_per_cu"] if valu else 1)
    cyc = ISSUE["valu_cycles_per_wave_inst"] if valu else ISSUE["lds_cycles_per_wave_inst"]
    peak = units * issue["clock_GHz"] / cyc            # G wave-instructions / s the chip can issue
    achieved = insts / k_s / 1e9
    hbm = {k: roof[k] for k in ("achieved", "peak", "unit", "frac", "algorithmic_bytes") if k in roof}
    hbm["bound"] = "hbm"
    for k in ("measured_copy_GBps", "frac_of_measured_copy", "plan_format_bytes", "plan_format_GBps", "step_frac", "rocprofv3"):
        if k in roof:
            hbm[k] = roof.pop(k)
    hbm["note"] = ("SURVEY 8(d) bytes / kernel time / 8 TB/s.  NOT the binding roofline: the kernel streams a pre-binned 6 B/event plan "
                   "out of the Infinity Cache (counter traffic < algorithmic bytes), so this fraction can exceed 1 against the measured "
                   "copy bandwidth")
    lead = {"bound": issue["bound"], "kernel": roof["kernel"], "achieved": round(achieved, 2), "peak": round(peak, 2),
            "unit": "Gwave-inst/s", "frac": round(achieved / peak, 4), "traffic": roof.get("traffic"),
            "insts_per_event": issue.get("valu_insts_per_event" if valu else "lds_insts_per_event"),
            "cycles_per_wave_inst": cyc, "issue_units": units, "clock_GHz": issue["clock_GHz"],
            "hbm_algorithmic_frac": hbm["frac"], "hbm_algorithmic": hbm,
            "bound_note": ("bound by " + issue["bound"] + ": " + ("VALU" if valu else "LDS") + " wave-instructions per launch (PMC, "
                           "profiles/pmc_latest.json, same kernel source) / kernel time, against issue_units x clock / cycles_per_wave_inst "
                           "(tools/ubench_valu_issue.hip, tools/ubench_lds.hip).  The HBM-priced figure is `hbm_algorithmic`.")}
    if "rocprofv3" in hbm:  # the committed rocprofv3 --kernel-trace --stats average of the same kernel, same source
        lead["rocprofv3_avg_us"] = hbm["rocprofv3"]["avg_us"]
        lead["rocprofv3_frac"] = round(insts / (hbm["rocprofv3"]["avg_us"] * 1e-6) / 1e9 / peak, 4)
    for k, v in roof.items():   # kernel times, traffic stamps, per-line notes
        if k not in lead and k not in ("achieved", "peak", "unit", "frac", "bound"):
            lead[k] = v
    return lead


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays, rank, world):
    """--dump-outputs: {name: tensor} -> DIR/<name>.npy (rank<r>_<name>.npy in an N-rank job), float32 / float64 as computed,
    at most DUMP_LIMIT_BYTES over all ranks."""
    import numpy as np

    host = {}
    for name, t in arrays.items():
        v = np.ascontiguousarray(t.detach().cpu().numpy())
        if v.dtype not in (np.float32, np.float64):
            raise SystemExit(f"--dump-outputs: {name} is {v.dtype}, not float32 / float64")
        host[name] = v
    total = world * sum(v.nbytes for v in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes over {world} rank(s) exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(dirname, exist_ok=True)
    for name, v in host.items():
        np.save(os.path.join(dirname, (f"rank{rank}_" if world > 1 else "") + name + ".npy"), v)


def base_line(R, value, ms_per_step, blocks, scaling, workload_cfg):
    a = R.args
    return {"metric": "Mevents/sec warped+IWE at 1280x720", "value": round(value, 2), "unit": "Mevents/s", "n_gpus": R.world,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic", "config": workload_cfg,
            "repeats": len(blocks), "timed_seconds": round(sum(blocks), 4),
            "block_ms": {"median": round(statistics.median(blocks) * 1e3, 4), "min": round(min(blocks) * 1e3, 4),
                         "max": round(max(blocks) * 1e3, 4)}}


def run_config2(R):
    import ctypes

    import numpy as np
    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip

    a, dev, rank, world = R.args, R.dev, R.rank, R.world
    lib = _hip.require_gpu()
    n = a.events or N_EVENTS
    t_ingest = time.perf_counter()
    ev, flow_np = synth_window(n, seed=rank, flow_max=a.flow_max)
    general = a.fractional or a.weighted
    if a.fractional:  # undistorted events: coordinates off the pixel grid, still inside the image
        rs_f = np.random.RandomState(4242 + rank)
        ev[:, 0] += rs_f.randint(0, 64, n) / 64.0
        ev[:, 1] += rs_f.randint(0, 64, n) / 64.0
    weights_np = np.random.RandomState(777 + rank).uniform(0.5, 1.5, n).astype(np.float32) if a.weighted else None
    if general:
        a.no_extras = True  # (the informative legs are the unit-weight compact plan's)
    if a.fractional:
        a.no_compact = True  # (the compact format holds integer source pixels; per-event weights ride along with it in plan order)
    ev_gpu = torch.from_numpy(ev).to(dev)
    flow = torch.from_numpy(flow_np).float().to(dev)
    if a.tile[0] <= 0:
        a.tile = list(ebos.event_plan.choose_tile((H, W), 32 if a.halo == 'auto' else a.halo))
    # plan build, timed host + device per window.  emit="compact" (ebos_plan_lean): what the unit-weight objective reads and
    # nothing else; the full build also leaves SoA x / y / dt / p and the permutation (per-event weights).  The first build of
    # a process also pays one-off allocator / code-object costs: the best of the later ones is reported.
    def time_build(emit):
        first = best = 0.0
        for attempt in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pl = ebos.EventPlan.build(ev_gpu, (H, W), "first", True, tile=tuple(a.tile), emit=emit)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            first = first or ms
            best = ms if attempt == 1 else min(best or ms, ms)
        return pl, first, best

    # the same window as the raw sensor columns a recording holds (src/data_loader/ccs.py:57-66: int16 x / y, int32 microseconds):
    # the lean build straight from them (EventPlan.build_raw) -- informative, beside the build from the reference's float64 [n, 4]
    # (a plain run keeps these builds too: ~7 ms of device work right before the warm-up, and the timed block has always started from
    # the state they leave.  Measured without them, the 200-step block read 0.4 - 2.5 % slower in nine alternated pairs out of nine;
    # ~5 ms of any other device work in their place closed the gap)
    plan_build_raw_ms = None
    if not general and not a.no_extras and not a.no_compact:
        raw_cols = [torch.from_numpy(v).to(dev) for v in (ev[:, 1].astype(np.int16), ev[:, 0].astype(np.int16),
                                                           np.rint(ev[:, 2] * 1e6).astype(np.int32), ev[:, 3].astype(np.uint8))]
        for attempt in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ebos.EventPlan.build_raw(*raw_cols, (H, W), "first", True, tile=tuple(a.tile), emit="compact")
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            plan_build_raw_ms = ms if attempt <= 1 else min(plan_build_raw_ms, ms)
        del raw_cols
    _, _, plan_build_full_ms = time_build("full")
    # (per-event weights are permuted like the events: the full build keeps the permutation)
    plan, plan_first_ms, plan_build_ms = time_build("full" if (a.no_compact or a.weighted) else "compact")
    ingest_s = time.perf_counter() - t_ingest  # host synthesis + upload + the timed plan builds: what a rank spends before its first step
    del ev_gpu
    a.halo_code = ebos.event_plan.resolve_halo(plan, a.halo)  # an int for the C ABI ('auto' -> EBOS_HALO_AUTO(32, 64 max|dt|))

    nws = int(lib.ebos_iwe_slab_workspace_bytes(H, W, a.tile[0], a.tile[1], a.halo_code, a.splits, 0, 0))
    ws = torch.zeros(nws, dtype=torch.uint8, device=dev)  # zero-filled once (spill section stays zero)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    moments = torch.empty((1, 2), dtype=torch.float64, device=dev)
    iwe = torch.empty((H, W), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: None if t is None else t.data_ptr()

    def compact_ptrs(pl):
        return pl._compact_ptrs() if (pl.compact and not a.no_compact) else (None, None, None)

    cptrs = compact_ptrs(plan)
    weight_p = ebos.event_plan._plan_weight(plan, torch.from_numpy(weights_np).to(dev)) if a.weighted else None  # plan order
    bytes_per_event = (6.0 if cptrs[0] else 12.0) + (4.0 if a.weighted else 0.0)

    def make_step(pl, fl, cp):
        def step():
            # one objective evaluation: tile accumulate -> slab combine (writes the IWE) -> variance
            _hip.check(lib.ebos_iwe_dense_slab_f32(P(pl.x), P(pl.y), P(pl.dt), P(weight_p) if pl is plan else None, *cp, P(pl.key_offsets), pl.n, P(fl),
                                                   H, W, a.tile[0], a.tile[1], a.halo_code, a.splits, 0, 0, P(ws), nws,
                                                   P(iwe), 1, 0, P(out), P(moments), P(pl.part_table), stream), "ebos_iwe_dense_slab")
        return step

    step = make_step(plan, flow, cptrs)
    blocks, kernel_ms = R.timed_blocks(step, lib, _hip.PROFILE_SLAB_ACCUMULATE,
                                       outputs=lambda: {"iwe": iwe, "variance": out, "moments": moments})
    elapsed = statistics.median(blocks)
    contrast = float(out.item())
    ranks_seen = R.gather({"rank": rank, "local_rank": R.local_rank, "device": torch.cuda.get_device_name(dev),
                           "events": plan.n, "contrast": contrast, "ingest_s": round(ingest_s, 2)})

    extras = {}
    # The informative legs (fwd + bwd, streams, rotating windows, solver iteration) run on rank 0 ONLY in an N-rank job: eight ranks
    # each synthesising eight more 10 M-event windows on the host, inside the driver's timeout, buy nothing -- `value` is measured
    # above, by every rank, and the other ranks wait at the final barrier.
    if a.full and not a.no_extras and (world == 1 or rank == 0):
        # (1) combine pass of the same step, timed the same way (outside `value`'s blocks)
        _hip.check(lib.ebos_profile_start_kernel(_hip.PROFILE_SLAB_COMBINE, 100), "profile")
        for _ in range(100):
            step()
        torch.cuda.synchronize()
        buf = (ctypes.c_float * 100)()
        got = lib.ebos_profile_stop(buf, 100)
        comb = [buf[i] for i in range(got)]
        if comb:
            extras["combine_kernel_ms"] = {"mean": round(statistics.mean(comb), 4), "min": round(min(comb), 4), "max": round(max(comb), 4)}
        else:
            extras["combine_kernel_ms"] = None

        # (2) forward + backward of the objective, direct C-ABI calls:
        #     slab forward + variance -> tile-private backward (variance gradient folded in from the moments)
        upstream = torch.full((1,), -1.0, dtype=torch.float32, device=dev)  # loss = -variance
        d_flow = torch.empty((2, H, W), dtype=torch.float32, device=dev)

        def step_fwd_bwd():
            step()
            _hip.check(lib.ebos_iwe_dense_tiled_bwd_f32(P(plan.x), P(plan.y), P(plan.dt), None, *cptrs, P(plan.key_offsets), plan.n,
                                                        P(flow), H, W, a.tile[0], a.tile[1], a.halo_code, 0, 0, P(iwe), None,
                                                        0, P(d_flow), None, P(moments), P(upstream), None, P(ws), nws,
                                                        P(plan.part_table) if a.splits == 0 else None, stream), "ebos_iwe_dense_tiled_bwd")

        for _ in range(5):
            step_fwd_bwd()
        torch.cuda.synchronize()
        reps = max(20, a.steps)
        _hip.check(lib.ebos_profile_start_kernel(_hip.PROFILE_TILED_BWD, reps), "profile")
        t1 = time.perf_counter()
        for _ in range(reps):
            step_fwd_bwd()
        torch.cuda.synchronize()
        fwdbwd_ms = (time.perf_counter() - t1) / reps * 1e3
        buf = (ctypes.c_float * reps)()
        got = lib.ebos_profile_stop(buf, reps)
        bwd_ms = [buf[i] for i in range(got)]
        extras["fwd_bwd_ms"] = round(fwdbwd_ms, 4)
        extras["fwd_bwd_mevents_per_s"] = round(n / fwdbwd_ms / 1e3, 2)
        # the same as ONE native call (ebos_variance_dense_job_f32: accumulate, combine, backward -- the backward kernel reduces the
        # variance partials itself, no finalize launch): what plan.variance_and_grad_dense / contrast_dense(...).backward() enqueue
        job = ebos.event_plan._dense_job(plan, (0, 0), a.halo_code, a.splits, False)
        out_j = torch.empty(1, dtype=torch.float32, device=dev)
        for _ in range(5):
            _hip.check(lib.ebos_variance_dense_job_f32(job.ref, P(flow), P(out_j), P(upstream), P(d_flow), stream), "ebos_variance_dense_job")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(reps):
            _hip.check(lib.ebos_variance_dense_job_f32(job.ref, P(flow), P(out_j), P(upstream), P(d_flow), stream), "ebos_variance_dense_job")
        torch.cuda.synchronize()
        job_ms = (time.perf_counter() - t1) / reps * 1e3
        extras["fwd_bwd_one_call_ms"] = round(job_ms, 4)
        extras["fwd_bwd_one_call_mevents_per_s"] = round(n / job_ms / 1e3, 2)
        # SURVEY 8(d) backward: 12 B/event (p unused) + read dIWE 4 B/px + write dflow 8 B/px
        extras["roofline_bwd"] = roofline_entry("iwe_dense_tiled_bwd_kernel", bwd_ms, 12.0 * plan.n + 12.0 * H * W)

        # (3) Informative only (NOT `value`): independent evaluations -- hypotheses of a sweep, windows of a recording -- in
        # flight on three HIP streams, each with its own workspace and outputs
        lanes = []
        for _ in range(3):
            lanes.append((torch.cuda.Stream(device=dev), torch.zeros(nws, dtype=torch.uint8, device=dev), torch.empty_like(iwe),
                          torch.empty_like(out), torch.empty_like(moments)))

        def overlapped(count):
            for k in range(count):
                st, ws_k, iwe_k, out_k, mom_k = lanes[k % 3]
                _hip.check(lib.ebos_iwe_dense_slab_f32(P(plan.x), P(plan.y), P(plan.dt), None, *cptrs, P(plan.key_offsets), plan.n,
                                                       P(flow), H, W, a.tile[0], a.tile[1], a.halo_code, a.splits, 0, 0,
                                                       P(ws_k), nws, P(iwe_k), 1, 0, P(out_k), P(mom_k), P(plan.part_table),
                                                       st.cuda_stream), "ebos_iwe_dense_slab")

        torch.cuda.synchronize()
        overlapped(6)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        cnt = 3 * max(10, a.steps)
        overlapped(cnt)
        torch.cuda.synchronize()
        overlapped_ms = (time.perf_counter() - t2) / cnt * 1e3
        extras["independent_evaluations_on_3_streams"] = {"ms_per_evaluation": round(overlapped_ms, 4),
                                                          "mevents_per_s": round(n / overlapped_ms / 1e3, 2),
                                                          "note": "informative, not `value`: 3 evaluations in flight, own workspaces"}
        del lanes

        # (the two legs below synthesise more windows on the host -- tens of seconds: they run in a ONE-rank job only, so that the
        # other ranks of an N-rank job never sit at the final barrier longer than the process group's timeout allows)
        if world == 1:
            # (4) cache-cold leg: distinct windows cycled so that the event stream of consecutive steps exceeds the 256 MiB
            # Infinity Cache (FETCH_SIZE counts Infinity-Cache hits as memory traffic: the resident-window number above is
            # measured in a cache-warm regime, this one streams from HBM)
            nrot = max(2, a.rotating_windows)
            rot = []
            for k in range(nrot):
                ev_k, fl_k = synth_window(n, seed=100 + k, flow_max=a.flow_max)
                pk = ebos.EventPlan.build(torch.from_numpy(ev_k).to(dev), (H, W), "first", True, tile=tuple(a.tile), emit="compact")
                rot.append((pk, torch.from_numpy(fl_k).float().to(dev)))
                del ev_k, fl_k
            rsteps = [make_step(pk, fk, compact_ptrs(pk)) for pk, fk in rot]
            for s_ in rsteps:
                s_()
            torch.cuda.synchronize()
            rounds = max(2, min(25, int(200 / nrot)))
            _hip.check(lib.ebos_profile_start_kernel(_hip.PROFILE_SLAB_ACCUMULATE, rounds * nrot), "profile")
            t3 = time.perf_counter()
            for _ in range(rounds):
                for s_ in rsteps:
                    s_()
            torch.cuda.synchronize()
            rot_ms = (time.perf_counter() - t3) / (rounds * nrot) * 1e3
            buf = (ctypes.c_float * (rounds * nrot))()
            got = lib.ebos_profile_stop(buf, rounds * nrot)
            rk = [buf[i] for i in range(got)]
            stream_bytes = sum((6.0 if pk.compact else 12.0) * pk.n + 8.0 * H * W for pk, _ in rot)
            algo = 12.0 * n + 12.0 * H * W
            extras["rotating_windows"] = {"n_windows": nrot, "bytes_streamed_per_cycle": stream_bytes,
                                          "ms_per_step": round(rot_ms, 4), "mevents_per_s": round(n / rot_ms / 1e3, 2),
                                          "kernel_ms": round(statistics.mean(rk), 4),
                                          "achieved": round(algo / (statistics.mean(rk) * 1e-3) / 1e9, 1),
                                          "frac": round(algo / (statistics.mean(rk) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                          "note": f"{nrot} distinct windows cycled ({stream_bytes / 2**20:.0f} MiB of plan + flow per cycle "
                                                  "> 256 MiB Infinity Cache): the HBM-streaming regime"}
            del rot, rsteps

        # (5) one Adam iteration of the patch-flow solver (the loop of src/solver/generative_max_likelihood.py:306-341; BASELINE
        # configs[3] shape): on this window and on a 2 M-event one, as four launches per iteration (ebos_cmax_patch_solve_f32) and as ONE
        # resident launch for the whole loop (ebos_cmax_patch_solve_resident_f32)
        if world == 1:
            try:
                from event_based_bos_amd.solver.fused_loop import FusedPatchLoop

                gh, gw = ebos.solver.patch_grid_shape((H, W), (24, 32), (24, 32))
                ev2, _ = synth_window(2_000_000, seed=7, flow=False)
                plan2 = ebos.EventPlan.build(torch.from_numpy(ev2).to(dev), (H, W), "first", True, tile=tuple(a.tile), emit="compact")
                del ev2
                leg = {"patch_grid": [gh, gw], "objective": "image_variance + 0.001 flow_norm, Adam, 200 iterations timed",
                       "note": "informative, not `value`: forward + backward + Adam step per iteration; run-time LDS windows (halo auto)"}
                # ... and BASELINE configs[0]'s size: 100 k events at 346x260 (99 tiles of 32 x 32, patches of 20 x 20)
                small = (260, 346)
                rs_s = np.random.RandomState(11)
                ev_s = np.stack([rs_s.randint(0, small[0], 100_000), rs_s.randint(0, small[1], 100_000),
                                 np.sort(rs_s.uniform(0, 0.5, 100_000)), rs_s.randint(0, 2, 100_000)], 1).astype(np.float64)
                plan_s = ebos.EventPlan.build(torch.from_numpy(ev_s).to(dev), small, "first", True, tile="auto", emit="compact")
                for tag, pl, patch in (("2M_events", plan2, (24, 32)), (f"{plan.n // 1_000_000}M_events", plan, (24, 32)),
                                       ("100k_events_346x260", plan_s, (20, 20))):
                    ent = {"events": pl.n}
                    g_h, g_w = ebos.solver.patch_grid_shape(pl.image_size, patch, patch)
                    for mode, res in (("four_launches", False), ("resident", True)):
                        sl = FusedPatchLoop(pl, patch, patch, torch.zeros((2, g_h, g_w)), 1.0, 0.001, 0.0, halo="auto", lr=0.1, capacity=260)
                        if res and not sl.resident_supported():
                            ent[mode] = {"unsupported": (lib.ebos_last_error() or b"").decode()}
                            continue
                        sl.run(10, resident=res)
                        torch.cuda.synchronize()
                        t4 = time.perf_counter()
                        losses = sl.run(200, resident=res)
                        torch.cuda.synchronize()
                        ent[mode] = {"us_per_iteration": round((time.perf_counter() - t4) / 200 * 1e6, 1), "ran_as": sl.last_run_mode,
                                     "last_loss": float(losses[-1])}
                        del sl
                    if "us_per_iteration" in ent.get("resident", {}):
                        ent["losses_identical"] = ent["resident"]["last_loss"] == ent["four_launches"]["last_loss"]
                    leg[tag] = ent
                # ... and what the shipped YAMLs select: iwe.blur_sigma > 0 (configs/cmax_hot_plate1.yaml: dense-flow
                # patches, blur 1) and the 2-DoF model with Adam and blur 3 (the reference's configs/hot_plate1.yaml:47,65,70), at
                # BASELINE configs[0]'s size and at 2 M events / 1280x720
                from event_based_bos_amd.solver.fused_loop import Fused2dofLoop

                for tag, pl, patch in (("100k_events_346x260", plan_s, (20, 20)), ("2M_events", plan2, (24, 32))):
                    g_h, g_w = ebos.solver.patch_grid_shape(pl.image_size, patch, patch)
                    for name, make in (("blur1_patch", lambda: FusedPatchLoop(pl, patch, patch, torch.zeros((2, g_h, g_w)), 1.0, 0.001, 0.0,
                                                                              halo="auto", lr=0.02, capacity=260, blur_sigma=1.0)),
                                       ("gradient_magnitude_patch", lambda: FusedPatchLoop(pl, patch, patch, torch.zeros((2, g_h, g_w)), 0.0, 0.001,
                                                                                           0.0, halo="auto", lr=0.02, capacity=260,
                                                                                           w_gradient_magnitude=1.0)),
                                       ("blur3_2dof", lambda: Fused2dofLoop(pl, torch.zeros(2), 1.0, halo="auto", lr=0.02, capacity=260,
                                                                            blur_sigma=3.0)),
                                       ("2dof", lambda: Fused2dofLoop(pl, torch.zeros(2), 1.0, halo="auto", lr=0.02, capacity=260))):
                        ent = {}
                        for mode, res in (("pipeline", False), ("resident", True)):
                            sl = make()
                            if res and not sl.resident_supported():
                                ent[mode] = {"unsupported": (lib.ebos_last_error() or b"").decode()}
                                continue
                            sl.run(10, resident=res)
                            torch.cuda.synchronize()
                            t4 = time.perf_counter()
                            losses = sl.run(200, resident=res)
                            torch.cuda.synchronize()
                            ent[mode] = {"us_per_iteration": round((time.perf_counter() - t4) / 200 * 1e6, 1), "ran_as": sl.last_run_mode,
                                         "last_loss": float(losses[-1])}
                            del sl
                        leg[tag][name] = ent
                # ... and events with fractional source coordinates (sub-pixel rectified or pre-warped): the patch loop's
                # launches run the dense route on the (x, y, dt) arrays, the resident launch the compact layout with the fractions
                for tag, (hh, ww), n_f, patch in (("2M_events", (H, W), 2_000_000, (24, 32)), ("100k_events_346x260", small, 100_000, (20, 20))):
                    rs_f = np.random.RandomState(13)
                    ev_f = np.stack([rs_f.randint(0, hh, n_f) + rs_f.randint(0, 64, n_f) / 64.0, rs_f.randint(0, ww, n_f) + rs_f.randint(0, 64, n_f) / 64.0,
                                     np.sort(rs_f.uniform(0, 0.5, n_f)), rs_f.randint(0, 2, n_f)], 1)
                    ev_f[:, :2] = np.clip(ev_f[:, :2], 0, [hh - 1, ww - 1])
                    pl_f = ebos.EventPlan.build(torch.from_numpy(ev_f).to(dev), (hh, ww), "first", True, tile="auto")
                    g_h, g_w = ebos.solver.patch_grid_shape((hh, ww), patch, patch)
                    ent = {}
                    for mode, res in (("pipeline", False), ("resident", True)):
                        sl = FusedPatchLoop(pl_f, patch, patch, torch.zeros((2, g_h, g_w)), 1.0, 0.001, 0.0, halo="auto", lr=0.02, capacity=260)
                        if res and not sl.resident_supported():
                            ent[mode] = {"unsupported": (lib.ebos_last_error() or b"").decode()}
                            continue
                        sl.run(10, resident=res)
                        torch.cuda.synchronize()
                        t4 = time.perf_counter()
                        losses = sl.run(200, resident=res)
                        torch.cuda.synchronize()
                        ent[mode] = {"us_per_iteration": round((time.perf_counter() - t4) / 200 * 1e6, 1), "ran_as": sl.last_run_mode,
                                     "last_loss": float(losses[-1])}
                        del sl
                    leg[tag]["patch_fractional_events"] = ent
                    del pl_f, ev_f
                leg["us_per_iteration"] = min(v["us_per_iteration"] for v in leg["2M_events"].values()
                                              if isinstance(v, dict) and "us_per_iteration" in v)
                # ... and a recording, window after window (solver.WindowPipeline: raw sensor columns in, windows side by side, one
                # resident launch each): the loop of the reference's configs/hot_plate1.yaml:47,65,70 (2-DoF, blur 3, Adam x 600) at
                # BASELINE configs[0]'s size, against the same solver called window by window
                try:
                    hh, ww = small
                    n_w, k_w = 100_000, 16
                    rs_p = np.random.RandomState(17)
                    store = ebos.data_loader.RawEventStore({"x": rs_p.randint(0, ww, n_w * k_w).astype(np.int16), "y": rs_p.randint(0, hh, n_w * k_w).astype(np.int16),
                                                            "t": np.sort(rs_p.randint(0, 8300 * k_w, n_w * k_w)).astype(np.int32) + 10_000_000,
                                                            "p": rs_p.randint(0, 2, n_w * k_w).astype(bool)})
                    wins = [(k * n_w, (k + 1) * n_w) for k in range(k_w)]
                    cfg_p = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "halo": "auto",
                             "cost_with_weight": {"image_variance": 1.0}, "iwe": {"method": "bilinear_vote", "blur_sigma": 3},
                             "optimizer": {"method": "Adam", "n_iter": 600, "parameters": {"lr": 0.05}}}
                    slv = ebos.solver.collections["contrast_maximization"]((hh, ww), (hh, ww), solver_config=cfg_p)
                    host = [store.load_event(*wnd) for wnd in wins[:3]]
                    slv.estimate(host[0])
                    torch.cuda.synchronize()
                    t4 = time.perf_counter()
                    for ev_w in host[1:]:
                        slv.estimate(ev_w)
                    torch.cuda.synchronize()
                    one_by_one = (time.perf_counter() - t4) / 2 * 1e3
                    pipe = ebos.solver.WindowPipeline(slv)   # (default: eight windows in flight on a sensor this small)
                    pipe.run(store, wins)
                    torch.cuda.synchronize()
                    t4 = time.perf_counter()
                    pipe.run(store, wins)
                    torch.cuda.synchronize()
                    leg["window_pipeline_346x260"] = {"objective": "2-DoF, blur 3, Adam x 600, 100 k events per window", "windows": k_w,
                                                      "ms_per_window": round((time.perf_counter() - t4) / k_w * 1e3, 2),
                                                      "ms_per_window_one_by_one": round(one_by_one, 2), "windows_in_flight": pipe.n_concurrent,
                                                      "tile": list(pipe.tile), "modes": sorted({m for wm in pipe.window_modes for m in wm})}
                    del store, pipe, slv
                except Exception as err:
                    leg["window_pipeline_346x260"] = {"error": repr(err)}
                extras["solver_iteration"] = leg
                del plan2, plan_s
            except Exception as err:  # the headline measurement must not depend on the solver layer
                extras["solver_iteration"] = {"error": repr(err)}

    if a.full:
        # next to the nominal peak, a bandwidth this box actually delivers -- a device-to-device copy of 1 GiB
        # (read + write bytes counted), best of 6
        a_buf = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        b_buf = torch.empty_like(a_buf)
        copy_gbs = 0.0
        for _ in range(6):
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            b_buf.copy_(a_buf)
            torch.cuda.synchronize()
            copy_gbs = max(copy_gbs, 2.0 * a_buf.numel() * 4 / (time.perf_counter() - t3) / 1e9)
        del a_buf, b_buf

    if rank == 0:
        ms_per_step = elapsed / a.steps * 1e3
        value = world * n * a.steps / elapsed / 1e6
        line = base_line(R, value, ms_per_step, blocks, "weak", {
            "workload": ("BASELINE configs[1]: 10M synthetic events, 1280x720 dense per-pixel flow U(-30,30), "
                         "variance cost, fwd objective (tile accumulate + slab combine + variance)") if (a.flow_max == FLOW_MAX and n == N_EVENTS and not general)
                        else (f"NOT the BASELINE workload: {n} events, flow U(-{a.flow_max:g},{a.flow_max:g})"
                              + (", source coordinates on a 1/64 px grid (12 B/event format, truncated flow look-up)" if a.fractional else "")
                              + (", per-event weights U(0.5, 1.5) (fixed point in units of the slice's max |w|)" if a.weighted else "")),
            "events_per_gpu": n, "events_in_plan": plan.n, "height": H, "width": W,
            "layout": (("compact SoA (u16 tile-local pixel + f32 dt, 6 B/event)" if cptrs[0] else "SoA f32 (x,y,dt), 12 B/event")
                       + (" + f32 weight in plan order" if a.weighted else ""))
                      + f", binned by source tile {a.tile[0]}x{a.tile[1]}, halo {a.halo}, splits {a.splits}",
            "parallelism": f"windows sharded, {world} rank(s), no collective"})
        if a.full:
            # 12 B/event (x, y, dt; p unused) + flow read (8 B/px) + IWE write (4 B/px)
            algo_bytes = (16.0 if a.weighted else 12.0) * plan.n + 12.0 * H * W  # (16 B/event with weights)
            format_bytes = bytes_per_event * plan.n + 12.0 * H * W  # what the plan format actually stores per event
            k_ms = statistics.mean(kernel_ms) if kernel_ms else float("nan")
            kname = "iwe_slab_accumulate_kernel<DENSE,DYN>" if a.halo == "auto" else "iwe_slab_accumulate_kernel"
            if not cptrs[0]:  # other instantiations: the committed counters are the compact unit-weight kernel's
                kname = "iwe_slab_accumulate_kernel<XY" + (",W>" if a.weighted else ">")
            elif a.weighted:
                kname = "iwe_slab_accumulate_kernel<W>"
            roof = roofline_entry(kname, kernel_ms, algo_bytes,
                                  {"measured_copy_GBps": round(copy_gbs, 1),
                                   "frac_of_measured_copy": round(algo_bytes / (k_ms * 1e-3) / 1e9 / copy_gbs, 4),
                                   "plan_format_bytes": format_bytes,
                                   "plan_format_GBps": round(format_bytes / (k_ms * 1e-3) / 1e9, 1),
                                   "step_frac": round(algo_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
            if "rotating_windows" in extras:
                roof["frac_rotating_windows"] = extras["rotating_windows"]["frac"]
            line["roofline"] = roof
            clock = device_clock_hz(dev)
            dyn = a.halo == "auto"
            line["roofline_issue"] = roofline_issue(kname, kernel_ms, clock, plan.n)
            if "roofline_bwd" in extras:
                extras["roofline_bwd_issue"] = roofline_issue("iwe_dense_tiled_bwd_kernel<DENSE,DYN>" if dyn else "iwe_dense_tiled_bwd_kernel",
                                                              [extras["roofline_bwd"]["kernel_ms"]], clock, plan.n)
                extras["roofline_bwd"] = lead_with_binding(extras["roofline_bwd"], extras["roofline_bwd_issue"])
            # the fractions side by side: what each one prices and what it says.  `roofline` leads with the roofline that BINDS (VALU issue /
            # LDS pipe, from the instruction counters of this kernel source); SURVEY 8(d)'s HBM accounting sits in roofline.hbm_algorithmic
            hbm_frac, plan_gbs, step_frac = roof["frac"], roof["plan_format_GBps"], roof["step_frac"]
            roof = line["roofline"] = lead_with_binding(roof, line["roofline_issue"])
            line["roofline_summary"] = {
                "hbm_algorithmic_frac": hbm_frac,                           # SURVEY 8(d) bytes (12 B/event + 12 H W) / kernel time / 8 TB/s
                "hbm_plan_format_frac": round(plan_gbs / HBM_PEAK_GBS, 4),  # the 6 B/event the compact plan really streams
                "hbm_counter_traffic_frac": (round(roof["traffic"] / (roof["kernel_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                                             if roof.get("traffic") else None),              # FETCH / WRITE counters of the same source
                "hbm_step_frac": step_frac,                                 # the WHOLE step (accumulate + combine + finalize) on the same bytes
                "hbm_rotating_windows_frac": roof.get("frac_rotating_windows"),              # plans cycled beyond the Infinity Cache
                "issue_frac": line["roofline_issue"].get("frac"),           # what binds: VALU issue / LDS pipe (roofline_issue)
                "binding": line["roofline_issue"].get("bound", "unknown (no counters for this kernel source)")}
        line["ranks_seen"] = ranks_seen
        line["plan_build_ms"] = round(plan_build_ms, 3)
        line["plan_build_kind"] = "lean (emit='compact': compact events + offsets only)" if plan.lean else "full (SoA + perm + compact)"
        line["plan_build_full_ms"] = round(plan_build_full_ms, 3)
        line["plan_build_first_call_ms"] = round(plan_first_ms, 2)
        # one evaluation of a FRESH window (BASELINE configs[1] read literally): plan build + one step
        line["value_incl_plan_build"] = round(n / (plan_build_ms + ms_per_step) / 1e3, 2)
        if plan_build_raw_ms is not None:  # ... when the window arrives as raw sensor columns (8 B/event instead of 32)
            line["plan_build_raw_columns_ms"] = round(plan_build_raw_ms, 3)
            line["value_incl_plan_build_raw_columns"] = round(n / (plan_build_raw_ms + ms_per_step) / 1e3, 2)
        # the regime a FRESH window sees: distinct windows cycled beyond the 256 MiB Infinity Cache (`value` is the resident window a
        # 600-iteration loop evaluates)
        if "rotating_windows" in extras:
            line["value_hbm_streaming"] = extras["rotating_windows"]["mevents_per_s"]
        # the three regimes of one workload, stated where the driver's line names the workload
        streaming = (format(line["value_hbm_streaming"], ".0f") if "value_hbm_streaming" in line
                     else "not measured (" + ("--no-extras" if a.full else "bench.py --full") + ")")
        line["config"]["workload"] += (f" | regimes [Mevents/s]: value = window resident from step to step (the CMax loop re-reads one window hundreds "
                                       f"of times) {line['value']:.0f}; value_hbm_streaming = distinct windows cycled beyond the Infinity Cache "
                                       f"{streaming}; value_incl_plan_build = a fresh window, plan build + one step "
                                       f"{line['value_incl_plan_build']:.0f}")
        line["contrast"] = contrast
        line.update(extras)
        if a.full and world == 1 and not a.no_cpu_baseline:
            sample = min(a.cpu_sample, n)
            line["cpu_baseline"] = cpu_baseline(ev, flow_np, sample)
            line["speedup_vs_cpu_port_f64"] = round(value / line["cpu_baseline"]["value"], 1)
            if sample < n:  # the same sample through the GPU path (outside the timed region)
                ps = ebos.EventPlan.build(torch.from_numpy(ev[:sample]).to(dev), (H, W), "first", True, tile=tuple(a.tile), emit="compact")
                make_step(ps, flow, compact_ptrs(ps))()
                gpu_c = float(out.item())
            else:
                gpu_c = contrast
            cpu_c = line["cpu_baseline"]["contrast_f64"]
            line["contrast_cpu"] = cpu_c
            line["contrast_gpu_same_sample"] = gpu_c
            line["contrast_rel_err"] = abs(gpu_c - cpu_c) / abs(cpu_c)
        print(json.dumps(line))


def cpu_baseline_gradmag(ev, flow, sample):
    """BASELINE configs[2] on the host: the oracle's torch-CPU restatement of warp + IWE + gradient-magnitude contrast (Sobel 3x3 / 8,
    replicate padding: src/utils/stat_utils.py:69-92, 117-139), forward and forward + backward (autograd), fp64, on a bounded sample."""
    import torch

    from oracle import ebos_oracle as O

    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    threads = min(avail, 8)
    torch.set_num_threads(threads)
    e = torch.from_numpy(ev[:sample])
    times_f, times_fb, contrast = [], [], None
    for rep in range(4):
        f = torch.from_numpy(flow).clone().requires_grad_(True)
        t0 = time.perf_counter()
        c = O.gradient_magnitude(O.iwe_dense(e, f, (H, W)))
        t1 = time.perf_counter()
        c.backward()
        t2 = time.perf_counter()
        times_f.append(t1 - t0)
        times_fb.append(t2 - t0)
        contrast = abs(float(c.item()))
        if sum(times_fb) > 40.0 and rep >= 1:
            break
    reps = len(times_f) - 1
    return {"value": round(sample / statistics.median(times_f[1:]) / 1e6, 3), "unit": "Mevents/s", "cores": threads, "host_cpus": avail,
            "kind": "port", "value_fwd_bwd": round(sample / statistics.median(times_fb[1:]) / 1e6, 3),
            "sample": (f"first {sample} events of the window, fwd warp + IWE + gradient magnitude (value_fwd_bwd: + autograd backward), "
                       f"torch-CPU fp64, median of {reps} after 1 warm-up"), "contrast_f64": contrast}


def run_config3(R):
    """BASELINE configs[2]: the config-2 window with the gradient-magnitude contrast (Sobel on the IWE).  A step = one evaluation of
    the objective on the resident plan (accumulate + combine + ONE Sobel pass that yields the value partials and the gradient image +
    finalize); informative: value + flow gradient as the one native call (ebos_gradient_magnitude_dense_job_f32)."""
    import ctypes

    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip

    a, dev, rank, world = R.args, R.dev, R.rank, R.world
    lib = _hip.require_gpu()
    n = a.events or N_EVENTS
    t_ingest = time.perf_counter()
    ev, flow_np = synth_window(n, seed=rank, flow_max=a.flow_max)
    flow = torch.from_numpy(flow_np).float().to(dev)
    if a.tile[0] <= 0:
        a.tile = list(ebos.event_plan.choose_tile((H, W), 32 if a.halo == "auto" else a.halo))
    plan = ebos.EventPlan.build(torch.from_numpy(ev).to(dev), (H, W), "first", True, tile=tuple(a.tile), emit="compact")
    halo_code = ebos.event_plan.resolve_halo(plan, a.halo)
    job = ebos.event_plan._dense_job(plan, (0, 0), halo_code, a.splits, False)
    d_iwe, partials, n_part = job.gm_buffers()
    out = torch.empty(1, dtype=torch.float32, device=dev)
    d_flow = torch.empty((2, H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ingest_s = time.perf_counter() - t_ingest
    stream = _hip.stream_ptr()
    P = lambda t: t.data_ptr()

    def step():
        _hip.check(lib.ebos_gradient_magnitude_dense_job_f32(job.ref, P(flow), P(out), None, None, None, P(d_iwe), P(partials), n_part, stream),
                   "ebos_gradient_magnitude_dense_job")

    def step_fwd_bwd():
        _hip.check(lib.ebos_gradient_magnitude_dense_job_f32(job.ref, P(flow), P(out), None, None, P(d_flow), P(d_iwe), P(partials), n_part, stream),
                   "ebos_gradient_magnitude_dense_job")

    blocks, sobel_ms = R.timed_blocks(step, lib, profile_kernel=_hip.PROFILE_GRADMAG_FUSED, outputs=lambda: {"gradient_magnitude": out})
    elapsed = statistics.median(blocks)
    contrast = float(out.item())
    ranks_seen = R.gather({"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", rank)), "device": str(dev), "units": 1,
                           "ingest_s": round(ingest_s, 2)})
    extras = {}
    if a.full and not a.no_extras and rank == 0:
        for _ in range(5):
            step_fwd_bwd()
        torch.cuda.synchronize()
        reps = max(50, a.steps)
        t1 = time.perf_counter()
        for _ in range(reps):
            step_fwd_bwd()
        torch.cuda.synchronize()
        fb_ms = (time.perf_counter() - t1) / reps * 1e3
        extras["fwd_bwd_one_call_ms"] = round(fb_ms, 4)
        extras["fwd_bwd_one_call_mevents_per_s"] = round(n / fb_ms / 1e3, 2)
        # the same through the Python API: (-plan.contrast_dense(flow, "gradient_magnitude")).backward()
        fl = flow.clone().requires_grad_(True)
        for _ in range(5):
            (-plan.contrast_dense(fl, "gradient_magnitude", halo=a.halo)).backward()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(reps):
            fl.grad = None
            (-plan.contrast_dense(fl, "gradient_magnitude", halo=a.halo)).backward()
        torch.cuda.synchronize()
        extras["python_contrast_dense_backward_us"] = round((time.perf_counter() - t1) / reps * 1e6, 1)
    if rank == 0:
        ms_per_step = elapsed / a.steps * 1e3
        value = world * n * a.steps / elapsed / 1e6
        line = base_line(R, value, ms_per_step, blocks, "weak", {
            "workload": ("BASELINE configs[2]: 10M synthetic events, 1280x720 dense per-pixel flow U(-30,30), gradient-magnitude cost "
                         "(Sobel 3x3 / 8 on the IWE), fwd objective (tile accumulate + slab combine + one Sobel pass)")
                        if (a.flow_max == FLOW_MAX and n == N_EVENTS) else f"NOT the BASELINE workload: {n} events, flow U(-{a.flow_max:g},{a.flow_max:g})",
            "events_per_gpu": n, "events_in_plan": plan.n, "height": H, "width": W,
            "layout": f"compact SoA (6 B/event), binned by source tile {a.tile[0]}x{a.tile[1]}, halo {a.halo}, splits {a.splits}",
            "parallelism": f"windows sharded, {world} rank(s), no collective"})
        if a.full:
            # SURVEY 8(d), cost kernels: 4 H W bytes read (+ 4 H W written for the gradient image)
            line["roofline"] = roofline_entry("gradmag_fused_kernel", sobel_ms, 8.0 * H * W,
                                              {"note": "the Sobel pass of the step: reads the IWE once, writes the gradient image once (SURVEY 8(d): "
                                                       "4 H W + 4 H W bytes); the step's event kernels are config 2's (bench.py --config 2 --full "
                                                       "carries their rooflines)",
                                               "step_frac_on_event_bytes": round((12.0 * plan.n + 12.0 * H * W) / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
        line["ranks_seen"] = ranks_seen
        line["contrast"] = contrast
        line.update(extras)
        if a.full and world == 1 and not a.no_cpu_baseline:
            sample = min(a.cpu_sample, n, 2_000_000)
            line["cpu_baseline"] = cpu_baseline_gradmag(ev, flow_np, sample)
            line["speedup_vs_cpu_port_f64"] = round(value / line["cpu_baseline"]["value"], 1)
            ps = ebos.EventPlan.build(torch.from_numpy(ev[:sample]).to(dev), (H, W), "first", True, tile=tuple(a.tile), emit="compact")
            gpu_c = float(ps.contrast_dense(flow, "gradient_magnitude", halo=a.halo).item())
            cpu_c = line["cpu_baseline"]["contrast_f64"]
            line["contrast_cpu"], line["contrast_gpu_same_sample"] = cpu_c, gpu_c
            line["contrast_rel_err"] = abs(gpu_c - cpu_c) / abs(cpu_c)
        print(json.dumps(line))


def run_config4(R):
    """64 windows x 2 M events, 30x40 patch-flow grid, windows round-robin over the ranks."""
    import numpy as np
    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip

    a, dev, rank, world = R.args, R.dev, R.rank, R.world
    lib = _hip.require_gpu()
    n = a.events or CONFIG4["events"]
    n_windows = a.windows or CONFIG4["windows"]
    mine = shard_for(4, rank, world, a)
    ph, pw = CONFIG4["patch"]
    sh, sw = CONFIG4["slide"]
    if a.tile[0] <= 0:
        a.tile = list(ebos.event_plan.choose_tile((H, W), 32 if a.halo == 'auto' else a.halo))
    if not lib.ebos_patch_fused_supported(a.tile[0], a.tile[1], 32 if a.halo == 'auto' else a.halo, sh, sw):
        raise SystemExit(f"config 4 needs a tile the grid-sampling kernels support, got {a.tile} halo {a.halo}")
    gh, gw = ebos.solver.patch_grid_shape((H, W), (ph, pw), (sh, sw))
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: None if t is None else t.data_ptr()
    t0 = time.perf_counter()
    plans, grids = [], []
    for wi in mine:
        ev, _ = synth_window(n, seed=wi, flow=False)
        plans.append(ebos.EventPlan.build(torch.from_numpy(ev).to(dev), (H, W), "first", True, tile=tuple(a.tile), emit="compact"))
        grids.append(torch.from_numpy(np.random.RandomState(100 + wi).uniform(-a.flow_max, a.flow_max, (2, gh, gw))).float().to(dev))
    torch.cuda.synchronize()
    ingest_s = time.perf_counter() - t0
    a.halo_code = ebos.event_plan.resolve_halo(plans[0], a.halo) if plans else 32
    splits = 1
    # The windows are independent (bos_event.py:144-220): like solver.WindowPipeline, a rank keeps three of them in flight on
    # three HIP streams, each with its own workspace and image -- the small combine / finalize kernels of one window run in
    # the wave slots the one-workgroup-per-CU accumulate kernel of another leaves free.  --streams 1: back to back.
    n_lanes = max(1, min(a.streams, len(plans)))
    nws = int(lib.ebos_iwe_slab_workspace_bytes(H, W, a.tile[0], a.tile[1], a.halo_code, splits, 0, 0))
    lanes = [(torch.cuda.Stream(device=dev) if n_lanes > 1 else None, torch.zeros(nws, dtype=torch.uint8, device=dev),
              torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((1, 2), dtype=torch.float64, device=dev))
             for _ in range(n_lanes)]
    outs = torch.empty(max(len(mine), 1), dtype=torch.float32, device=dev)

    def eager_step():
        main = torch.cuda.current_stream(dev)
        if n_lanes > 1:
            for st, _, _, _ in lanes:
                st.wait_stream(main)
        for k, (pl, g) in enumerate(zip(plans, grids)):
            st, ws, iwe, moments = lanes[k % n_lanes]
            _hip.check(lib.ebos_iwe_patch_slab_f32(*pl._compact_ptrs(), P(pl.key_offsets), pl.n, P(g), gh, gw, ph, pw, sh, sw, H, W,
                                                   a.tile[0], a.tile[1], a.halo_code, splits, 0, 0, P(ws), nws, P(iwe), 1, 0,
                                                   outs.data_ptr() + 4 * k, P(moments), P(pl.part_table),
                                                   st.cuda_stream if st is not None else main.cuda_stream),
                       "ebos_iwe_patch_slab")
        if n_lanes > 1:
            for st, _, _, _ in lanes:
                main.wait_stream(st)

    # One pass is 3 launches x the rank's windows through a 35-argument C call each: enqueued from Python it is HOST-bound (0.86 ms
    # of host time for 64 windows against < 0.8 ms of GPU work).  The pass is therefore captured once as a HIP graph (fork / join
    # over the side streams) and replayed -- the launch-bound inner loop the solver's FusedPatchLoop replays the same way.
    # --no-graph: enqueue every call from Python.
    def measure_enqueue(fn):
        enq = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            enq.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
        return statistics.median(enq) * 1e3

    # (what runs before the timed block runs in a plain run too: it is the state the timed block has always started from)
    eager_step()  # (first call: reserves LDS, creates workspaces' state)
    torch.cuda.synchronize()
    eager_enqueue_ms = measure_enqueue(eager_step)
    step, graphed = eager_step, False
    if not a.no_graph and plans and a.batch <= 0:  # (the batched entry below needs no graph: one C call per pass)
        try:
            graph = torch.cuda.CUDAGraph()
            cap = torch.cuda.Stream(device=dev)
            cap.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.graph(graph, stream=cap):
                eager_step()
            torch.cuda.synchronize()
            step, graphed = graph.replay, True
        except Exception as e:  # capture not possible: the eager pass stays
            sys.stderr.write(f"[bench] config 4: graph capture failed ({type(e).__name__}: {e}); eager pass\n")
            torch.cuda.synchronize()
    first = outs[:len(mine)].clone()
    # --batch B (default 16): the rank's windows go through ebos_iwe_slab_batch_f32, B windows per accumulate / combine / finalize
    # launch; the combine / finalize passes of one batch run on a second stream beside the accumulate pass of the next.
    # Same kernels' bodies, same bits as the per-window calls (checked below).  --batch 0: per-window calls.
    batches = []
    if a.batch > 0 and plans:
        tail = torch.cuda.Stream(device=dev)
        # (one call per --batch windows; inside a call the library launches 16 windows at a time and joins the tail stream at its end)
        for b0 in range(0, len(plans), a.batch):
            batches.append(ebos.SlabBatch(plans[b0:b0 + a.batch], grids[b0:b0 + a.batch], patch=((ph, pw), (sh, sw)), halo=a.halo,
                                          splits=splits))

        def batch_step():  # accumulate, combine and finalize passes back to back on the current stream (--tail-stream: the latter two beside the next accumulate pass)
            for bt in batches:
                bt.run(tail_stream=tail.cuda_stream if a.tail_stream and not a.no_tail_stream else None)

        batch_step()
        torch.cuda.synchronize()
        got = torch.cat([bt.variances for bt in batches])
        if not torch.equal(first, got):
            raise SystemExit(f"config 4: batched contrasts differ from the per-window calls: {first[:4].tolist()} vs {got[:4].tolist()}")
        step, graphed = batch_step, False

    def variances():  # what a pass computed: one contrast per window of this rank
        return torch.cat([bt.variances for bt in batches]) if batches else outs[:len(mine)]

    blocks, _ = R.timed_blocks(step, lib, _hip.PROFILE_SLAB_ACCUMULATE, launches_per_step=max(len(mine), 1), profile_blocks=0,
                               outputs=lambda: {"variance": variances()})
    elapsed = statistics.median(blocks)
    res = {int(wi): float(v) for wi, v in zip(mine, variances().tolist())}
    kernel_ms = []
    if a.full:
        if graphed and not torch.equal(first, outs[:len(mine)]):
            raise SystemExit("config 4: the replayed graph's contrasts differ from the eager pass")
        host_enqueue_ms = measure_enqueue(step)
        # roofline leg: the kernel timed on ONE stream, back to back (a dispatch that shares the chip with its neighbours' kernels
        # has no clean begin-to-end time)
        import ctypes
        nrec = max(1, min(len(plans), 16))
        _hip.check(lib.ebos_profile_start_kernel(_hip.PROFILE_SLAB_ACCUMULATE, nrec), "profile")
        for k, (pl, g) in enumerate(zip(plans[:nrec], grids[:nrec])):
            _, ws, iwe, moments = lanes[0]
            _hip.check(lib.ebos_iwe_patch_slab_f32(*pl._compact_ptrs(), P(pl.key_offsets), pl.n, P(g), gh, gw, ph, pw, sh, sw, H, W,
                                                   a.tile[0], a.tile[1], a.halo_code, splits, 0, 0, P(ws), nws, P(iwe), 1, 0,
                                                   outs.data_ptr() + 4 * k, P(moments), P(pl.part_table), stream), "ebos_iwe_patch_slab")
        torch.cuda.synchronize()
        buf = (ctypes.c_float * nrec)()
        got = lib.ebos_profile_stop(buf, nrec)
        kernel_ms = [buf[i] for i in range(got)]
    seen = R.gather({"rank": rank, "local_rank": R.local_rank, "device": torch.cuda.get_device_name(dev),
                     "windows": len(mine), "events": int(sum(p.n for p in plans)), "contrasts": res, "ingest_s": round(ingest_s, 2)})
    if rank == 0:
        total_events = n * n_windows
        ms_per_step = elapsed / a.steps * 1e3
        value = total_events * a.steps / elapsed / 1e6
        line = base_line(R, value, ms_per_step, blocks, "strong", {
            "workload": (f"BASELINE configs[3]: {n_windows} time windows x {n} events, {gh}x{gw} patch-flow grid "
                         f"(patch {ph}x{pw}, slide {sh}x{sw}) -> 1280x720, variance cost, fwd objective per window"
                         + ("" if a.flow_max == FLOW_MAX else f"; NOT the BASELINE flow: cells U(-{a.flow_max:g},{a.flow_max:g})")),
            "windows_total": n_windows, "events_per_window": n, "height": H, "width": W,
            "layout": f"compact SoA 6 B/event, tile {a.tile[0]}x{a.tile[1]}, halo {a.halo}; flow sampled from the patch grid per tile",
            "parallelism": f"windows round-robin over {world} rank(s) (bos_event.py:144-220), no collective"})
        if a.full:
            algo = 6.0 * n + 4.0 * H * W + 8.0 * gh * gw  # per launch: compact events (6 B) + IWE write + the patch grid (no dense flow field)
            dyn = a.halo == "auto"
            line["roofline_issue"] = roofline_issue("iwe_slab_accumulate_kernel<GRID,DYN>" if dyn else "iwe_slab_accumulate_kernel<GRID>",
                                                    kernel_ms, device_clock_hz(dev), n)
            line["roofline"] = roofline_entry("iwe_slab_accumulate_kernel<GRID,DYN>" if dyn else "iwe_slab_accumulate_kernel<GRID>", kernel_ms, algo,
                                              {"note": "kernel timed on one stream, back to back",
                                               "ms_per_window_in_step": round(ms_per_step / max(len(mine), 1), 5), "streams": n_lanes,
                                               **survey_priced(12.0 * n + 4.0 * H * W + 8.0 * gh * gw, kernel_ms)})
            line["roofline"] = lead_with_binding(line["roofline"], line["roofline_issue"])
        line["ranks_seen"] = [{k: v for k, v in s.items() if k != "contrasts"} for s in seen]
        merged = {}
        for s in seen:
            merged.update(s["contrasts"])
        line["windows_evaluated"] = len(merged)
        line["contrast_first_windows"] = [merged[k] for k in sorted(merged)[:4]]
        line["ingest_s_this_rank"] = round(ingest_s, 2)
        if a.full:
            line["host_enqueue_ms_per_step"] = round(host_enqueue_ms, 4)
        line["pass_is_a_replayed_hip_graph"] = graphed
        line["windows_per_launch"] = min(a.batch, 16) if batches else 1
        line["host_enqueue_ms_per_step_eager"] = round(eager_enqueue_ms, 4)
        print(json.dumps(line))


def run_config5(R):
    """512 2-DoF hypotheses over one 50 M-event window replicated on every rank, hypotheses in blocks."""
    import numpy as np
    import torch

    import event_based_bos_amd as ebos
    from event_based_bos_amd import _hip

    a, dev, rank, world = R.args, R.dev, R.rank, R.world
    lib = _hip.require_gpu()
    n = a.events or CONFIG5["events"]
    g0, g1 = CONFIG5["grid"]
    tm = CONFIG5["theta_max"]
    # optuna grid sampler over [-30, 30) x [-30, 30) (generative_max_likelihood.py:238-255), 32 x 16 points
    gx, gy = np.arange(-tm, tm, 2 * tm / g0), np.arange(-tm, tm, 2 * tm / g1)
    grid = np.stack(np.meshgrid(gx, gy, indexing="ij"), -1).reshape(-1, 2)
    mine = shard_for(5, rank, world, a)
    if a.tile[0] <= 0:
        a.tile = list(ebos.event_plan.choose_tile((H, W), 32 if a.halo == 'auto' else a.halo))
    t0 = time.perf_counter()  # (ingest = host synthesis of the window + upload + plan build: what a rank spends before its first step)
    ev, _ = synth_window(n, seed=0, flow=False)  # the SAME window on every rank
    plan = ebos.EventPlan.build(torch.from_numpy(ev).to(dev), (H, W), "first", True, tile=tuple(a.tile), emit="compact")
    torch.cuda.synchronize()
    ingest_s = time.perf_counter() - t0
    del ev
    th = torch.from_numpy(grid[mine]).float().to(dev)
    res = {}

    def step():
        res["v"] = plan.variance_2dof(th, chunk=16, halo=a.halo, n_streams=a.streams)

    blocks, _ = R.timed_blocks(step, lib, _hip.PROFILE_SLAB_ACCUMULATE, launches_per_step=max(len(mine), 1), profile_blocks=0,
                               outputs=lambda: {"variance": res["v"]})
    elapsed = statistics.median(blocks)
    v = res["v"].cpu().numpy()
    kernel_ms = []
    if a.full:
        # roofline leg: the timed sweep keeps three hypotheses in flight on three streams, where a dispatch's begin-to-end time
        # includes the time it shares the chip with its neighbours; the kernel is therefore timed on ONE stream, back to back
        import ctypes
        # (the accumulate pass is one PERSISTENT launch per chunk of 16 hypotheses: its time is quoted per hypothesis)
        nrec = min(len(mine), 64)
        _hip.check(lib.ebos_profile_start_kernel(_hip.PROFILE_SLAB_ACCUMULATE, nrec), "profile")
        plan.variance_2dof(th[:nrec], chunk=16, halo=a.halo, n_streams=1)
        torch.cuda.synchronize()
        buf = (ctypes.c_float * nrec)()
        got = lib.ebos_profile_stop(buf, nrec)
        sizes = [min(16, nrec - k0) for k0 in range(0, nrec, 16)]
        kernel_ms = [buf[i] / sizes[i] for i in range(min(got, len(sizes)))]
    seen = R.gather({"rank": rank, "local_rank": R.local_rank, "device": torch.cuda.get_device_name(dev),
                     "hypotheses": len(mine), "events": plan.n, "ingest_s": round(ingest_s, 2),
                     "variances": {int(k): float(x) for k, x in zip(mine, v)}})
    if rank == 0:
        K = grid.shape[0]
        ms_per_step = elapsed / a.steps * 1e3
        value = float(n) * K * a.steps / elapsed / 1e6  # event-warps per second, whole job
        line = base_line(R, value, ms_per_step, blocks, "strong", {
            "workload": f"BASELINE configs[4]: {K}-hypothesis 2-DoF flow sweep ({g0}x{g1} grid over [-{tm:g},{tm:g})^2) over {n} events, "
                        "1280x720, variance cost per hypothesis",
            "hypotheses_total": K, "events": n, "height": H, "width": W,
            "layout": f"compact SoA 6 B/event, tile {a.tile[0]}x{a.tile[1]}, halo {a.halo}; event window replicated per rank",
            "parallelism": f"hypotheses in contiguous blocks over {world} rank(s) (generative_max_likelihood.py:229-236), no collective"})
        line["unit_note"] = "Mevents/s counts event-warps: every hypothesis warps and splats every event"
        if a.full:
            algo = 6.0 * plan.n + 4.0 * H * W  # per hypothesis launch: compact events (6 B) + IWE write (theta is two floats)
            dyn = a.halo == "auto"
            key5 = "iwe_slab_accumulate_batch_kernel<UNIFORM,DYN>" if dyn else "iwe_slab_accumulate_batch_kernel<UNIFORM>"
            line["roofline"] = roofline_entry(key5, kernel_ms, algo,
                                              {"note": "the persistent accumulate pass (one launch per 16 hypotheses) timed on one stream, per hypothesis "
                                                       "(the timed sweep overlaps three streams)",
                                               "ms_per_hypothesis_in_sweep": round(ms_per_step / max(len(mine), 1), 5),
                                               **survey_priced(12.0 * plan.n + 4.0 * H * W, kernel_ms)})
            # SURVEY 8(d) prices config 5 per pass of K hypotheses: 16 B/event ONCE per K + 4 H W K B of images.  The tile-private path
            # re-streams the plan once per hypothesis; on that accounting (K = 64, one rank's block of the 8-GPU job) it moves
            k_pass = 64
            per_pass = 16.0 * plan.n + 4.0 * H * W * k_pass
            k_ms_mean = statistics.mean(kernel_ms) if kernel_ms else float("nan")
            line["roofline"]["per_pass_of_K"] = {"K": k_pass, "algorithmic_bytes_per_pass": per_pass,
                                                 "achieved": round(per_pass / (k_pass * k_ms_mean * 1e-3) / 1e9, 1),
                                                 "frac": round(per_pass / (k_pass * k_ms_mean * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                                 "note": "SURVEY 8(d): 16 B/event per pass of K hypotheses + 4 H W K; the kernel is instruction-bound "
                                                         "(roofline_issue), K hypotheses per event read would save the shared decode only: "
                                                         "profiles/r03_multi_hypothesis_ablation.txt"}
            line["roofline_issue"] = roofline_issue(key5, kernel_ms, device_clock_hz(dev), plan.n)
            line["roofline"] = lead_with_binding(line["roofline"], line["roofline_issue"])
        line["ranks_seen"] = [{k: x for k, x in s.items() if k != "variances"} for s in seen]
        merged = {}
        for s in seen:
            merged.update(s["variances"])
        best = max(merged, key=merged.get)
        line["hypotheses_evaluated"] = len(merged)
        line["best_hypothesis"] = {"index": int(best), "theta": grid[best].tolist(), "variance": merged[best]}
        line["ingest_s_this_rank"] = round(ingest_s, 2)
        print(json.dumps(line))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus > 1 and "RANK" not in os.environ:
        return launch_ranks(args, argv)  # before torch / HIP is touched in this process
    if args.dry_run:
        return dry_run(args)
    R = Rank(args)
    {2: run_config2, 3: run_config3, 4: run_config4, 5: run_config5}[args.config](R)
    if R.distributed:
        R.dist.barrier()
        R.dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
