#!/usr/bin/env python3
"""Benchmark of the MI355X GICP engine on BASELINE.json's headline workload.

Metric (BASELINE.json): GICP iterations/sec + ms-to-converge on 5M <-> 5M points, and the
final-transform Frobenius error against the PCL CPU path (the oracle restatement).

One *step* = one complete GICP align loop (PCL Registration::align as re-run by
GICPAlignment::iterate(), /root/reference/src/GICPAlignment.cpp:111-121) over clouds resident
in HBM whose grids and covariances are cached (the first align, in warmup, builds them and is
reported separately as ms_to_converge_first).  value = outer GICP iterations of all timed
steps / timed seconds.  With N GPUs the same 5M <-> 5M problem is sharded by source point
ranges (strong scaling); every rank runs the resident pass server and the per-pass super rows go
into every rank's IPC-mapped device buffer over xGMI, where a totaler wave per rank takes the
fixed-order total (--transport xgmi, default, r05), or through a node-wide shared-memory segment
that every host totals (--transport shm), or one RCCL all-gather per pass (--transport rccl).

A plain run sets up, warms up, times the K steps and prints the result line (the headline roofline row
comes from the timed steps' own server events).  --full adds every other leg after the timed steps: the
kernel-time and pass-bench rooflines, Gauss-Newton mode, the new-clouds / cold-pair / GICPState cycles,
the C5 pass, the FOD rows, the CPU baselines and the parity against the oracle.  --dump-outputs DIR
writes what the last timed align returned as DIR/<name>.npy.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--n-source S] [--n-target T] [--full]
                       [--dump-outputs DIR]
       (N > 1: this script starts its own N ranks, or runs under torch.distributed.run)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md chip table)
# Algorithmic bytes per unit, SURVEY.md 8(d) / BASELINE.md section 2 (DESIGN.md "Kernels"):
#   BFGS objective pass, per accepted correspondence: s 12 + q 12 + M (6 x fp32) 24 + idx 4 = 52 B
#     (the engine stores M as 6 fp64 for bit parity with PCL's Matrix3d: 72 B actually read per
#      correspondence, reported as a labelled second figure)
#   correspondence + Mahalanobis, per source point per outer iteration: s 12 + Cs 24 + NN 12 + Ct 24 = 72 B
#   k-NN(20) covariance, per point: (k + 1) x 12 + 24 = 276 B
FDF_BYTES_SURVEY = 52
FDF_BYTES_STORED = 72
CORR_BYTES = 72
COV_BYTES = lambda k: (k + 1) * 12 + 24  # noqa: E731


# BASELINE.json configs (C1, the cube plumbing case, is the unit-test fixture, not a bench line)
CONFIGS = {
    "C2": dict(n_source=100_000, n_target=100_000, max_iter=100, fixed=False, occlusion=0.0,
               text="C2: 100k-pt synthetic scan vs 100k-pt CAD-sampled cloud, k=20"),
    "C3": dict(n_source=1_000_000, n_target=1_000_000, max_iter=50, fixed=True, occlusion=0.0,
               text="C3: 1M-pt scan vs 1M-pt CAD, exactly 50 GICP iterations (delta test off)"),
    "C4": dict(n_source=5_000_000, n_target=5_000_000, max_iter=100, fixed=False, occlusion=0.0,
               text="C4: 5M-pt scan vs 5M-pt CAD-sampled synthetic aero part"),
    "C5": dict(n_source=20_000_000, n_target=5_000_000, max_iter=100, fixed=False, occlusion=0.25,
               text="C5: 20M-pt scan (25% of the surface occluded) vs 5M-pt CAD, guess=I, full converge"),
    # C4 with scan content that has no CAD partner: 4 % clutter 5-30 cm off the
    # part, 40k points in 40 debris blobs 0.5-5 cm off it -- the gate rejects part of every sweep
    "C4F": dict(n_source=5_000_000, n_target=5_000_000, max_iter=100, fixed=False, occlusion=0.0,
                clutter=0.04, debris=40_000,
                text="C4F: 5M-pt scan with 4% clutter + 40 debris blobs (no CAD partner) vs 5M-pt CAD"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)  # the 1-NN cell lists are built by aligns 3-4
    ap.add_argument("--config", default="C4", choices=sorted(CONFIGS),
                    help="BASELINE.json workload (default C4: the metric's 5M<->5M)")
    ap.add_argument("--n-source", type=int, default=None, help="override the config's scan size")
    ap.add_argument("--n-target", type=int, default=None, help="override the config's CAD size")
    ap.add_argument("--cpu-sample", type=int, default=500_000,
                    help="points per cloud of the bounded CPU-baseline sample (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=1)
    ap.add_argument("--oracle-full", type=int, default=1,
                    help="1 = run the oracle on the full workload on the box's granted CPU share "
                         "(min(OMP_NUM_THREADS, affinity) threads: the thread-share CPU baseline + full-size "
                         "frob_vs_oracle; rank 0, N = 1 only)")
    ap.add_argument("--pmc-json", default=os.path.join(ROOT, "scripts", "pmc_summary_c4.json"))
    ap.add_argument("--gn-steps", type=int, default=5,
                    help="timed aligns of the opt-in Gauss-Newton mode (MGICP_SOLVER_GN; 0 = skip)")
    ap.add_argument("--fod-cpu-sample", type=int, default=500_000,
                    help="points of the CPU-oracle sample for the FOD-side rows (0 = skip those rows)")
    ap.add_argument("--no-events", action="store_true",
                    help="skip the kernel-time (HIP event) leg")
    ap.add_argument("--pass-bench", type=int, default=5,
                    help="roofline leg of the resident pass server: this many server launches of "
                         "--pass-bench-passes back-to-back objective passes each (0: off)")
    ap.add_argument("--pass-bench-passes", type=int, default=50)
    ap.add_argument("--prof-steps", type=int, default=3,
                    help="aligns of the kernel-time leg (HIP events around every kernel family)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch + rendezvous of every rank only (no GPU, libmgicp.so not loaded)")
    ap.add_argument("--cold-pairs", type=int, default=3,
                    help="repeats of the reference's call pattern (fresh context, set_source, set_target, align, "
                         "align: GICPState / testRunWithCov) for the cold_pair field (0 = skip)")
    ap.add_argument("--c5-leg", type=int, default=1,
                    help="C4 only: the in-align pass roofline at C5 (20M scan: the streams exceed the 256 MiB "
                         "Infinity Cache) measured in this run (0 = skip)")
    ap.add_argument("--transport", default="xgmi", choices=["xgmi", "shm", "rccl"],
                    help="N > 1: per-pass super rows into every rank's IPC-mapped device buffer over xGMI with a "
                         "totaler wave per rank (r05 default), or through the node-wide shared host segment "
                         "(every host totals), or one RCCL all-gather per pass")
    ap.add_argument("--no-rccl", action="store_true",
                    help="N > 1: skip RCCL (the path a failed ncclCommInitRank falls back to: RCCL-free shards, "
                         "target covariances on every rank, rows through the segment / xGMI)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg: kernel-time (HIP event) and pass-bench "
                         "rooflines, Gauss-Newton mode, new-clouds / cold-pair / GICPState cycles, the C5 pass, the "
                         "FOD rows, the CPU baselines and the oracle parity (--cpu-sample, --oracle-full, "
                         "--gn-steps, --fod-cpu-sample, --no-events, --pass-bench, --prof-steps, --cold-pairs and "
                         "--c5-leg shape those legs and mean nothing without --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed align returned as DIR/<name>.npy (rank 0): "
                         "final_transformation (4x4 f32), iteration_transformations (iterations x 4x4 f32), "
                         "align_result (f64: converged, iterations, accepted correspondences)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        # a plain run does only what `value` needs: set up, warm up, the timed steps, the result line
        args.cpu_sample = args.fod_cpu_sample = args.oracle_full = args.gn_steps = 0
        args.pass_bench = args.cold_pairs = args.c5_leg = 0
        args.no_events = True
    cfg = CONFIGS[args.config]
    args.n_source = args.n_source or cfg["n_source"]
    args.n_target = args.n_target or cfg["n_target"]
    args.max_iter, args.fixed, args.occlusion, args.cfg_text = cfg["max_iter"], cfg["fixed"], cfg["occlusion"], cfg["text"]
    args.clutter, args.debris = cfg.get("clutter", 0.0), cfg.get("debris", 0)
    return args


def gen_clouds(args, n_source=None, n_target=None):
    """the config's synthetic scan-vs-CAD clouds (synth.scan_vs_cad), optionally at another size"""
    from leica_point_cloud_processing_amd import synth

    ns, nt = n_source or args.n_source, n_target or args.n_target
    debris = int(round(args.debris * ns / args.n_source)) if args.debris else 0
    return synth.scan_vs_cad(ns, nt, occlusion=args.occlusion, clutter=args.clutter, debris=debris)


def dist_setup(args):
    """RANK / WORLD_SIZE / MASTER_* come from torch.distributed.run or from launch_ranks below; the
    control plane is leica_point_cloud_processing_amd.parallel.Rendezvous (torch is never imported
    in a process that uses libmgicp.so: see parallel.py for the two-HIP-runtime hazard)."""
    from leica_point_cloud_processing_amd.parallel import Rendezvous

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    return world, rank, local, Rendezvous(rank, world)


def _free_port() -> int:
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` without torchrun: this parent starts N fresh
    child processes of this script -- one rank per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in
    their environment -- relays rank 0's stdout (the JSON line) and exits non-zero if any child
    does.  The parent itself never loads libmgicp.so or touches HIP: it only spawns and waits
    (children are separate programs, not an exec of this process)."""
    import subprocess
    import threading

    port, ctrl = _free_port(), _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "MGICP_CTRL_PORT": str(ctrl)})
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr.fileno(),
                                      text=True, start_new_session=False))
    lines = []

    def relay():
        for line in procs[0].stdout:
            lines.append(line)
            sys.stdout.write(line)
            sys.stdout.flush()

    t = threading.Thread(target=relay, daemon=True)
    t.start()
    rc = 0
    alive = set(range(n))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                sys.stderr.write(f"bench.py: rank {r} exited with {code}; stopping the other ranks\n")
                for o in alive:
                    procs[o].terminate()  # the exact children this parent started
        time.sleep(0.05)
    t.join(timeout=10)
    return rc


def dry_run(args, world, rank, pg):
    """--dry-run: the launch and rendezvous of every rank (the shared-segment name and a 128-byte id
    broadcast, barrier, max-over-ranks timer) without loading libmgicp.so -- the CPU test of the
    N > 1 launch path."""
    name = pg.broadcast(f"/mgicp_dry_{os.getpid()}".encode() if rank == 0 else None)
    uid = pg.broadcast(bytes(range(128)) if rank == 0 else None)
    pg.barrier()
    joined = pg.allreduce_max(float(rank)) + 1
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "ranks_joined": int(joined),
                          "uid_ok": uid == bytes(range(128)), "shm_name": name.decode(),
                          "local_rank": int(os.environ.get("LOCAL_RANK", "0"))}))


def cpu_baseline(args, n, threads):
    """Oracle (PCL 1.8.1 restatement, single thread like PCL GICP) on a bounded sample of the
    same synthetic workload; per-iteration cost grows at least linearly with N, so the
    5M-equivalent rate is reported as sample_rate * n / 5M (an upper bound for the CPU)."""
    from oracle import ref

    scan, cad, _ = gen_clouds(args, n, n)
    g = ref.RefGICP(threads=threads)
    g.set_source(scan)
    g.set_target(cad)
    T, info = g.align()
    rate = info["iterations"] / info["t_loop_s"]
    return rate, info, T, (scan, cad)


def host_info():
    """The GPU box's host CPU as the CPU baseline states it."""
    model = None
    try:
        import subprocess

        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.startswith("Model name:"):
                model = line.split(":", 1)[1].strip()
                break
    except Exception:  # noqa: BLE001 -- lscpu absent: report what python sees
        pass
    share = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS")
    # the box grants a CPU share (OMP_NUM_THREADS) smaller than the machine (nproc)
    usable = min(share, int(omp)) if omp and omp.isdigit() and int(omp) > 0 else share
    return {"lscpu_model": model, "nproc": os.cpu_count(), "sched_affinity": share,
            "OMP_NUM_THREADS": omp, "threads_used": usable,
            "thread_share": f"{usable} of {os.cpu_count()} hardware threads (the box's granted share)"}


def oracle_full(scan, cad, threads, max_iter, fixed, guess=None):
    """The oracle on the FULL workload with the box's granted thread share (OpenMP): the CPU
    baseline at the config's own size (no scaling) and the full-size final-transform parity."""
    from oracle import ref

    g = ref.RefGICP(threads=threads, max_iterations=max_iter, fixed_iterations=fixed)
    g.set_source(scan)
    g.set_target(cad)
    t = time.perf_counter()
    T, info = g.align(want_trace=True)
    info["wall_s"] = time.perf_counter() - t
    return T, info


def fod_rows(eng, scan, cad, T_final, n_cpu):
    """SURVEY 8f rows 2 and 4 around the GICP path, at the config's size, host buffers in/out:
    VoxelGrid of the scan with the state machine's leaf (10 x max resolution,
    LeicaStateMachine.cpp:61-65) and SegmentDifferences of the GICP-transformed scan against the
    CAD cloud with the launch file's threshold (4e-3 * voxelize_factor 0.1,
    LeicaStateMachine.cpp:184-188); CPU oracle timed on a bounded sample of each."""
    from leica_point_cloud_processing_amd.cloud import PointCloudRGB
    from oracle import ref

    rows = {}
    cloud = PointCloudRGB.from_xyz(scan, rgb=0xff808080)
    t = time.perf_counter()
    res = max(eng.cloud_resolution(scan), eng.cloud_resolution(cad))
    ms_res = 1e3 * (time.perf_counter() - t) / 2
    leaf = float(np.float32(10 * res))
    ms = []
    for _ in range(3):
        t = time.perf_counter()
        out = eng.voxel_grid(cloud, leaf)
        ms.append(1e3 * (time.perf_counter() - t))
    vg = {"ms": round(min(ms), 3), "points": len(scan), "leaf_m": leaf, "voxels": len(out),
          "Mpts_per_s": round(len(scan) / min(ms) / 1e3, 1),
          "note": "wall time from host records (32 B/pt) to host records, incl. PCIe both ways"}
    thr = 4e-3 * 0.1
    ms = []
    for _ in range(3):
        t = time.perf_counter()
        keep, cnt = eng.segment_differences(scan, cad, thr, T=T_final)
        ms.append(1e3 * (time.perf_counter() - t))
    sd = {"ms": round(min(ms), 3), "points": len(scan), "target_points": len(cad), "sqr_threshold": thr,
          "kept": cnt, "Mpts_per_s": round(len(scan) / min(ms) / 1e3, 1),
          "note": "wall time incl. H2D of both clouds, target grid build and the keep-mask D2H"}
    if n_cpu > 0:
        n_cpu = min(n_cpu, len(scan))
        sub = cloud.points[:n_cpu]
        t = time.perf_counter()
        ref.voxel_grid(sub, leaf)
        vg["cpu_baseline"] = {"ms": round(1e3 * (time.perf_counter() - t), 3), "points": n_cpu, "cores": 1,
                              "kind": "port", "Mpts_per_s": round(n_cpu / (time.perf_counter() - t) / 1e6, 2)}
        moved = (scan[:n_cpu] @ T_final[:3, :3].T + T_final[:3, 3]).astype(np.float32)
        csub = cad[: max(1, n_cpu * len(cad) // len(scan))]
        t = time.perf_counter()
        ref.segment_differences(moved, csub, thr)
        dt = time.perf_counter() - t
        sd["cpu_baseline"] = {"ms": round(1e3 * dt, 3), "points": n_cpu, "target_points": len(csub), "cores": 1,
                              "kind": "port", "Mpts_per_s": round(n_cpu / dt / 1e6, 2)}
    rows["voxel_grid"] = vg
    rows["segment_differences"] = sd
    rows["cloud_resolution_ms"] = round(ms_res, 3)
    return rows


def dump_outputs(out_dir, eng, T, max_iter):
    """--dump-outputs: what the last timed align handed its caller, as .npy files (a few hundred
    bytes; the clouds are seeded, so two builds run with the same arguments compare file for file)."""
    r = eng.last_result
    trace = eng.debug_trace(max_iter + 1)  # the transform after every outer iteration of that align
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "final_transformation.npy"), np.asarray(T, np.float32))
    np.save(os.path.join(out_dir, "iteration_transformations.npy"),
            np.asarray(trace, np.float32).reshape(-1, 4, 4))
    np.save(os.path.join(out_dir, "align_result.npy"),
            np.array([r["converged"], r["iterations"], r["n_corr"]], np.float64))


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    world, rank, local, pg = dist_setup(args)
    if args.dry_run:
        dry_run(args, world, rank, pg)
        return
    from leica_point_cloud_processing_amd.engine import GICPEngine

    t_gen = time.time()
    scan, cad, T_true = gen_clouds(args)
    t_gen = time.time() - t_gen

    if world > 1:
        # a rank whose exchange never delivers fails the align within 30 s (library default 120 s), so the
        # xGMI probe below can fall back to the host segment within the run
        os.environ.setdefault("MGICP_REMOTE_DEADLINE_S", "30")
    # ms_create and its parts: dlopen of libmgicp.so (the HIP runtime and RCCL libraries
    # it links), the HIP runtime's device init (first HIP call), then mgicp_create (streams, events, the pinned
    # pass words and the BAR command block)
    import ctypes as _ct

    from leica_point_cloud_processing_amd import _lib as _mlib

    t_c = time.perf_counter()
    _lib_h = _mlib.load()
    t_dl = time.perf_counter()
    _ndev = _ct.c_int(0)
    _lib_h.mgicp_device_count(_ct.byref(_ndev))
    t_rt = time.perf_counter()
    eng = GICPEngine(device=local, max_iter=args.max_iter, fixed_iterations=int(args.fixed))
    t_ctx = time.perf_counter()
    ms_create = 1e3 * (t_ctx - t_c)
    create_parts = {"ms_dlopen_libmgicp_hip_rccl": round(1e3 * (t_dl - t_c), 3),
                    "ms_hip_runtime_device_init": round(1e3 * (t_rt - t_dl), 3),
                    "ms_mgicp_create_context": round(1e3 * (t_ctx - t_rt), 3)}
    transport = "local"
    transport_notes = []
    if world > 1:
        # RCCL (target covariances), the node-wide row segment and the xGMI exchange, each agreed by every
        # rank; RCCL or xGMI failing degrades to the next form instead of failing the run (VERDICT r05
        # item 7, parallel.setup_transport)
        from leica_point_cloud_processing_amd.parallel import setup_transport

        probe = (np.ascontiguousarray(scan[::20]), np.ascontiguousarray(cad[::20]))
        tr = setup_transport(eng, pg, world, rank, args.transport, args.n_source, probe=probe,
                             force_rccl_fail=bool(args.no_rccl))
        transport = tr["transport"]
        transport_notes = tr["notes"]
    eng.set_source_xyz(scan)
    eng.set_target_xyz(cad)

    # warmup: the first align builds grids + covariances (ms-to-converge incl. one-time work)
    first = None
    warm = []  # aligns 1..W after set_*, the 1-NN cell lists built by aligns 3-4
    for w in range(max(1, args.warmup)):
        t_w = time.perf_counter()
        eng.align()
        t_w = time.perf_counter() - t_w
        if w == 0:
            first = dict(eng.last_result)
        vs = eng.vlist_stats() if world == 1 else {}
        warm.append({"align": w + 1, "ms_wall": round(1e3 * t_w, 3), "ms_loop": round(eng.last_result["ms_loop"], 3),
                     "lists": vs.get("lists"), "requested": vs.get("requested")})
    iters_per_align = eng.last_result["iterations"]
    kt_cov = eng.kernel_times()  # profiling is off until now; filled below
    # the target's 1-NN cell lists after the warmup aligns (built by their sweeps; the timed aligns
    # then find every cell they query listed or rejected -- DESIGN.md "1-NN cell lists")
    vlist = eng.vlist_stats()

    # timed region: K full align loops with no per-launch instrumentation (pre-launched, gated
    # objective passes on).  align() is host-synchronous (it returns with T on the host after its
    # stream drained), so the barrier on each side is the whole device synchronisation.
    st0 = eng.pass_stats()
    eng.server_time(reset=True)
    pg.barrier()
    t0 = time.perf_counter()
    total_iters = 0
    n_evals = 0
    for _ in range(args.steps):
        T_timed = eng.align()
        total_iters += eng.last_result["iterations"]
        n_evals += eng.last_result["n_evals"]
    pg.barrier()
    dt = time.perf_counter() - t0
    dt = pg.allreduce_max(dt)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, eng, T_timed, args.max_iter)
    # which pass path the timed aligns ran: every pass on the resident server,
    # none taken over by a launched pass; and the server's own in-align time per pass (two HIP events
    # per server launch on the engine stream -- launch to exit, host round trips between passes
    # included)
    st1 = eng.pass_stats()
    pass_stats_timed = {k: st1[k] - st0[k] for k in ("server_launches", "server_passes", "launched_passes",
                                                      "takeovers", "server_denied")}
    pass_stats_timed["bar_commands"] = st1["bar_commands"]
    srv_inalign = eng.server_time(reset=True)
    # kernel-time leg (roofline): the same aligns with HIP events on the engine's stream around
    # every kernel family (objective passes sampled every 8th); events turn the gating off, so each
    # pass is timed from its own start -- the gated launches of the timed leg also hold the host's
    # BFGS decision time, which is not kernel time
    kt = eng.kernel_times()  # all zero until a profiled leg ran
    if not args.no_events:
        eng.set_profiling(True)
        for _ in range(max(1, args.prof_steps)):
            eng.align()
        kt = eng.kernel_times()
        eng.set_profiling(False)
    # roofline leg of the pass the aligns run on one GPU: the resident pass server (one
    # launch holding part of the streams on chip across passes) in its timing form -- P passes of
    # one state back to back, chained on the device -- bracketed by HIP events on the engine's
    # stream; rocprofv3 lists it as fdf_server_kernel<true> (duration / P = one pass).  Beside it the
    # launched form (one fdf_soa_kernel per pass) over the same correspondences.
    srv = None
    if args.pass_bench > 0 and world == 1:
        x0 = np.zeros(6)
        P = args.pass_bench_passes
        ms_srv = [eng.debug_pass_bench(x0, P, 0)[0] for _ in range(args.pass_bench)]
        ms_lau = [eng.debug_pass_bench(x0, P, 1)[0] for _ in range(args.pass_bench)]
        srv = {"ms_per_pass": float(np.mean(ms_srv)), "ms_per_pass_runs": [round(v, 5) for v in ms_srv],
               "launched_ms_per_pass": float(np.mean(ms_lau)), "passes_per_launch": P,
               "launches": args.pass_bench}
    T_final = eng.getFinalTransformation()
    trace_final = eng.debug_trace(args.max_iter + 1)  # per-iteration transforms of the last timed align
    result = dict(eng.last_result)

    # opt-in Gauss-Newton mode on the same cached grids / covariances (every rank takes part:
    # one 80-double all-reduce per outer iteration)
    gn = None
    if args.gn_steps > 0:
        from leica_point_cloud_processing_amd import _lib

        eng.setSolver(_lib.MGICP_SOLVER_GN)
        eng.align()  # warmup
        eng.set_profiling(not args.no_events)
        pg.barrier()
        t0 = time.perf_counter()
        gn_iters = 0
        for _ in range(args.gn_steps):
            eng.align()
            gn_iters += eng.last_result["iterations"]
        pg.barrier()
        gdt = pg.allreduce_max(time.perf_counter() - t0)
        gkt = eng.kernel_times()
        eng.set_profiling(False)
        T_gn = eng.getFinalTransformation()
        mom_ms = gkt["gn_moments"]["avg_ms"]
        n_sh = args.n_source // world
        gn = {
            "solver": "MGICP_SOLVER_GN (moment pass + host Gauss-Newton; not PCL's trajectory)",
            "value": round(gn_iters / gdt, 3),
            "unit": "iterations/s",
            "ms_per_align": round(1e3 * gdt / args.gn_steps, 3),
            "iterations_per_align": eng.last_result["iterations"],
            "device_passes_per_align": eng.last_result["n_evals"],
            "frob_vs_pcl_bfgs_mode": float(np.linalg.norm(T_gn.astype(np.float64) - T_final.astype(np.float64))),
            "err_vs_truth_gn": float(np.abs(T_gn.astype(np.float64) @ T_true - np.eye(4)).max()),
            "err_vs_truth_pcl_bfgs": float(np.abs(T_final.astype(np.float64) @ T_true - np.eye(4)).max()),
            "kernels": {
                "correspond": gkt["correspond"],
                # per source point of the shard: src 16 + flag 4 + nn 4 + Cs 48 + tgt 16 + Ct 48
                "gn_moments": {**gkt["gn_moments"], "algorithmic_bytes": 136 * n_sh,
                               "achieved_GBps": (136 * n_sh / (mom_ms * 1e-3) / 1e9) if mom_ms else None},
            },
        }
        eng.setSolver(_lib.MGICP_SOLVER_PCL_BFGS)

    # a fresh engine in this (now warm) process: set_target + set_source + align wall time from
    # host buffers to T on the host -- what a long-running caller pays for every new cloud pair --
    # with covariance-kernel events on (the timed region above runs with cached covariances)
    eng2 = None
    new_clouds = None
    if rank == 0 and world == 1 and args.full:
        # wall time as a caller sees it (no instrumentation: the profiling mode turns the resident
        # pass server off), then the covariance kernels' times from a profiled repeat
        eng2 = GICPEngine(device=local, max_iter=args.max_iter, fixed_iterations=int(args.fixed),
                          options={"target_cache": 0})  # new clouds: no target state from earlier engines
        t_n = time.perf_counter()
        eng2.set_target_xyz(cad)  # r04: uploads, builds the grid, starts the covariances (2nd stream)
        t_t = time.perf_counter()
        eng2.set_source_xyz(scan)  # the same for the source, beside the target's covariances
        t_s = time.perf_counter()
        eng2.align()
        t_a = time.perf_counter()
        new_clouds = {"ms_wall": round(1e3 * (t_a - t_n), 3),
                      "ms_set_target": round(1e3 * (t_t - t_n), 3), "ms_set_source": round(1e3 * (t_s - t_t), 3),
                      "ms_align": round(1e3 * (t_a - t_s), 3),
                      **{k: round(eng2.last_result[k], 3) for k in ("ms_upload", "ms_prep", "ms_loop")}}
        eng2.set_profiling(True)
        eng2.set_target_xyz(cad)  # new clouds: the covariances are recomputed under events
        eng2.set_source_xyz(scan)
        eng2.align()
        kt_cov = eng2.kernel_times()
        eng2.close()

    # the reference's own call pattern: GICPState builds a fresh GICPAlignment every
    # cycle and aligns once (LeicaStateMachine.cpp:149-150), the unit test adds one iterate()
    # (test_gicp_alignment.cpp:124); fineAlignment sets the source, then the target
    # (GICPAlignment.cpp:89-90).  So: a fresh context, set_source, set_target, align, align -- no cell
    # lists exist in either align.  Each align's loop (ms_loop: the iterations alone, from the
    # correspondence sweep of iteration 1 to T) and its wall time from the host's view.
    cold_pair = None
    if rank == 0 and world == 1 and args.cold_pairs > 0:
        reps = []
        for _ in range(args.cold_pairs):
            # cold: the target cache off (no state from an earlier engine: see gicpstate_cycles for it on)
            e4 = GICPEngine(device=local, max_iter=args.max_iter, fixed_iterations=int(args.fixed),
                            options={"target_cache": 0})
            t_a = time.perf_counter()
            e4.set_source_xyz(scan)
            t_b = time.perf_counter()
            e4.set_target_xyz(cad)
            t_c2 = time.perf_counter()
            aligns = []
            for _a in range(2):
                t_0 = time.perf_counter()
                T_cp = e4.align()
                t_1 = time.perf_counter()
                lr = e4.last_result
                aligns.append({"ms_wall": round(1e3 * (t_1 - t_0), 3), "ms_loop": round(lr["ms_loop"], 3),
                               "ms_prep": round(lr["ms_prep"], 3), "iterations": lr["iterations"],
                               "objective_passes": lr["n_evals"],
                               "loop_iterations_per_s": round(lr["iterations"] / (lr["ms_loop"] * 1e-3), 2)})
            reps.append({"ms_set_source": round(1e3 * (t_b - t_a), 3), "ms_set_target": round(1e3 * (t_c2 - t_b), 3),
                         "ms_to_converge_first": round(1e3 * (t_c2 - t_a) + aligns[0]["ms_wall"], 3),
                         "align": aligns, "frob_vs_timed": float(np.linalg.norm(
                             T_cp.astype(np.float64) - T_final.astype(np.float64)))})
            e4.close()

        def med(f):
            return round(float(np.median([f(r) for r in reps])), 3)

        cold_pair = {
            "pattern": ("fresh context; set_source, set_target (GICPAlignment.cpp:89-90); align (fineAlignment, :96); "
                        "align (iterate, :116) -- GICPState's cycle (LeicaStateMachine.cpp:149-150) plus the unit "
                        "test's iterate(); no 1-NN cell lists are used in either align"),
            "first_align_ms_loop": med(lambda r: r["align"][0]["ms_loop"]),
            "first_align_loop_iterations_per_s": med(lambda r: r["align"][0]["loop_iterations_per_s"]),
            "first_align_ms_wall": med(lambda r: r["align"][0]["ms_wall"]),
            "second_align_ms_loop": med(lambda r: r["align"][1]["ms_loop"]),
            "second_align_loop_iterations_per_s": med(lambda r: r["align"][1]["loop_iterations_per_s"]),
            "second_align_ms_wall": med(lambda r: r["align"][1]["ms_wall"]),
            "ms_to_converge_first": med(lambda r: r["ms_to_converge_first"]),
            "ms_to_converge_pair": med(lambda r: r["ms_to_converge_first"] + r["align"][1]["ms_wall"]),
            "median_of": len(reps),
            "repeats": reps,
        }

    # r05: the same call pattern as GICPState runs it scan after scan -- a fresh engine per cycle, the same
    # CAD target every time -- with the library's target cache (default on): cycle 1 builds the target's
    # grid and covariances, cycles 2+ adopt them.  No engine here runs the 3+ aligns that build the 1-NN
    # cell lists, so no cycle uses lists (the cache carries lists only once some engine built them).  A
    # new scan's (source's) upload, grid and covariances are paid every cycle.
    gicpstate = None
    if rank == 0 and world == 1 and args.cold_pairs > 0:
        GICPEngine.release_cache()
        cyc = []
        for c in range(5):
            e6 = GICPEngine(device=local, max_iter=args.max_iter, fixed_iterations=int(args.fixed),
                            options={"target_cache": 1})  # r06: the cache is opt-in
            t_a = time.perf_counter()
            e6.set_source_xyz(scan)
            e6.set_target_xyz(cad)
            t_b = time.perf_counter()
            adopted = e6.cache_stats()["adopted"]
            al = []
            for _a in range(2):
                t_0 = time.perf_counter()
                T_c = e6.align()
                t_1 = time.perf_counter()
                lr = e6.last_result
                al.append({"ms_wall": round(1e3 * (t_1 - t_0), 3), "ms_loop": round(lr["ms_loop"], 3),
                           "iterations": lr["iterations"],
                           "loop_iterations_per_s": round(lr["iterations"] / (lr["ms_loop"] * 1e-3), 2)})
            e6.close()
            cyc.append({"cycle": c + 1, "target_adopted": bool(adopted), "ms_set_clouds": round(1e3 * (t_b - t_a), 3),
                        "ms_to_converge_first": round(1e3 * (t_b - t_a) + al[0]["ms_wall"], 3), "align": al,
                        "frob_vs_timed": float(np.linalg.norm(T_c.astype(np.float64) -
                                                              T_final.astype(np.float64)))})
        GICPEngine.release_cache()
        steady = cyc[1:]
        gicpstate = {
            "pattern": ("GICPState scan after scan (LeicaStateMachine.cpp:141-150): a fresh engine per cycle, "
                        "set_source + set_target (the same CAD points every cycle), align + iterate; the library's "
                        "target cache hands the CAD cloud's grid and covariances from one cycle's engine to the "
                        "next (adopted only when the uploaded points are equal bit for bit); no cell lists"),
            "steady_first_align_ms_loop": round(float(np.median([c["align"][0]["ms_loop"] for c in steady])), 3),
            "steady_first_align_loop_iterations_per_s": round(float(np.median(
                [c["align"][0]["loop_iterations_per_s"] for c in steady])), 2),
            "steady_ms_to_converge_first": round(float(np.median([c["ms_to_converge_first"] for c in steady])), 3),
            "cycles": cyc,
        }

    # the in-align pass past the Infinity Cache: at C4 ~248 MB of streamed bytes
    # per pass fit the 256 MiB MALL; C5's 20M-point scan streams ~1.3 GB per pass from HBM
    c5_pass = None
    if rank == 0 and world == 1 and args.c5_leg > 0 and args.config == "C4":
        from leica_point_cloud_processing_amd import synth

        c5 = CONFIGS["C5"]
        t_g = time.perf_counter()
        s5, c5t, _ = synth.scan_vs_cad(c5["n_source"], c5["n_target"], occlusion=c5["occlusion"])
        gen5 = time.perf_counter() - t_g
        e5 = GICPEngine(device=local, max_iter=c5["max_iter"])
        e5.set_source_xyz(s5)
        e5.set_target_xyz(c5t)
        del s5, c5t
        e5.align()
        e5.align()
        e5.server_time(reset=True)
        e5.align()
        e5.align()
        st5 = e5.server_time(reset=True)
        m5 = e5.last_result["n_corr"]
        if st5["passes"] > 0:
            ach5 = FDF_BYTES_SURVEY * m5 / (st5["ms_per_pass"] * 1e-3) / 1e9
            c5_pass = {"kernel": "fdf_server_kernel<false, 4> (in-align, C5 20M-pt scan vs 5M CAD)",
                       "bound": "hbm", "achieved": round(ach5, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": round(ach5 / HBM_PEAK_GBS, 4), "bytes_per_unit": FDF_BYTES_SURVEY,
                       "units_per_launch": int(m5), "avg_launch_ms": st5["ms_per_pass"],
                       "launches_timed": st5["passes"], "server_in_align": st5, "data_gen_s": round(gen5, 2),
                       "note": ("per pass, 2 aligns after 2 untimed ones; ~1.3 GB of the 1.44 GB of streams per pass "
                                "come from HBM (C4's fit the Infinity Cache): the HBM-bound form of the headline kernel")}
        e5.close()

    if rank != 0:
        eng.close()
        return
    value = total_iters / dt
    n_shard = args.n_source // world
    m_shard = result["n_corr"] / world
    fdf_ms = kt["fdf"]["avg_ms"]
    pmc = {}
    if os.path.exists(args.pmc_json):
        with open(args.pmc_json) as f:
            pmc = json.load(f)
        if not (pmc.get("n_source") == args.n_source and pmc.get("world") == world):
            pmc = {}
    pmc_k = pmc.get("kernels", {})

    def roof(name, unit_bytes, units, avg_ms, launches_timed, pmc_key, note):
        """one roofline record: algorithmic bytes (SURVEY 8d per-unit figure x units per launch) /
        average launch time (HIP events on the engine's stream during the timed region)"""
        alg = unit_bytes * units
        ach = alg / (avg_ms * 1e-3) / 1e9 if avg_ms and avg_ms > 0 else None
        tr = pmc_k.get(pmc_key, {})
        return {"kernel": name, "bound": "hbm", "achieved": round(ach, 1) if ach else None,
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4) if ach else None,
                "traffic": tr.get("hbm_bytes_per_launch"), "traffic_note": tr.get("correction"),
                "bytes_per_unit": unit_bytes, "units_per_launch": int(units),
                "algorithmic_bytes_per_launch": int(alg), "avg_launch_ms": avg_ms,
                "launches_timed": launches_timed, "numerator": note}

    traffic_src = os.path.relpath(args.pmc_json, ROOT) if pmc else None
    if srv_inalign["passes"] > 0:
        # the headline: the pass exactly as the timed aligns ran it -- fdf_server_kernel<false, 4>, one
        # launch per BFGS run, duration / passes it served
        pass_ms, pass_n = srv_inalign["ms_per_pass"], srv_inalign["passes"]
        pass_name = ("fdf_server_kernel<false, 4> (resident pass server as the timed aligns ran it: BFGS objective "
                     "pass, dominant; launch duration / passes served, host BFGS round trip between passes "
                     "included)")
        pass_pmc = "fdf_server_kernel"
    elif srv is not None:
        # no server ran in the timed aligns (another context held the device): the timing form
        pass_ms, pass_n = srv["ms_per_pass"], srv["passes_per_launch"] * srv["launches"]
        pass_name = ("fdf_server_kernel (resident pass server, timing form fdf_server_kernel<true>, duration / "
                     "passes_per_launch = one pass)")
        pass_pmc = "fdf_server_kernel"
    else:
        pass_ms, pass_n = fdf_ms, kt["fdf"]["count"]
        pass_name = "fdf_soa_kernel (BFGS objective pass, dominant: ~48 launches per outer iteration)"
        pass_pmc = "fdf_soa_kernel"
    roofline = roof(pass_name, FDF_BYTES_SURVEY, m_shard, pass_ms, pass_n, pass_pmc,
                    "SURVEY 8d / BASELINE.md: 52 B per accepted correspondence per pass (M as 6 fp32)")
    roofline["launches"] = n_evals
    roofline["traffic_source"] = (f"{traffic_src}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the timing form "
                                  "(fdf_server_kernel<true, 4>, per pass), committed from the last profiled GPU job "
                                  "(profiles/<round>/final/pmc_summary.json), not measured in this run"
                                  if traffic_src else None)
    roofline["pass_stats_timed"] = pass_stats_timed
    if srv is not None:
        tf_frac = (FDF_BYTES_SURVEY * m_shard / (srv["ms_per_pass"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                   if srv["ms_per_pass"] > 0 else None)
        roofline["timing_form"] = {
            **srv,
            "frac_52B": round(tf_frac, 4) if tf_frac else None,
            "timing": (f"HIP events on the engine stream around {srv['launches']} server launches of "
                       f"{srv['passes_per_launch']} back-to-back passes each (mgicp_debug_pass_bench mode 0: the "
                       "aligns' pass chained on the device by a global ticket instead of the host's next command, "
                       "i.e. without the host BFGS round trip) over the last timed align's correspondences; "
                       "~31 % of the bytes are register / LDS resident, the rest stream from HBM / Infinity Cache"),
        }
    if srv_inalign["passes"] > 0:
        roofline["timing"] = (f"HIP events on the engine stream around each of the {srv_inalign['launches']} resident-"
                              f"server launches of the timed aligns ({srv_inalign['passes']} passes, "
                              f"{srv_inalign['ms']:.3f} ms in total): in-align time per pass = launch duration / "
                              "passes served, the host's BFGS step between passes included")
        roofline["server_in_align"] = srv_inalign
    elif srv is not None:
        roofline["timing"] = roofline["timing_form"]["timing"]
    else:
        roofline["timing"] = ("HIP events on the engine stream around every 8th objective pass of the timed region "
                              "(identical work per pass; sampling keeps the events' own cost out of value)")
    # the 72 B the pass reads per correspondence (M stored as 6 fp64 for bit parity) per pass time: a
    # read RATE, not an HBM fraction -- ~31 % of those bytes are register / LDS resident across the
    # passes of a BFGS run and C4's streamed rest fits the Infinity Cache
    stored_rate = round(FDF_BYTES_STORED * m_shard / (pass_ms * 1e-3) / 1e9, 1) if pass_ms else None
    stored = {"kernel": pass_name, "bytes_per_unit": FDF_BYTES_STORED, "units_per_launch": int(m_shard),
              "avg_launch_ms": pass_ms, "read_rate_GBps": stored_rate,
              "note": ("72 B per accepted correspondence per pass (M as 6 fp64) / pass time: the pass's read rate "
                       "from registers, LDS, Infinity Cache and HBM together -- not a fraction of HBM peak "
                       "(31 % of the bytes are on chip); the HBM-bound form is rooflines.fdf_52B_c5_past_infinity_cache")}
    launched = roof("fdf_soa_kernel (launched form, one launch per pass)", FDF_BYTES_SURVEY, m_shard,
                    srv["launched_ms_per_pass"] if srv else fdf_ms, pass_n, "fdf_soa_kernel",
                    "52 B per accepted correspondence per pass")
    corr_ms = kt["correspond"]["avg_ms"] + kt["compact"]["avg_ms"]
    # per cloud: the logged k-NN launch plus its (rare) register-list hand-off launch, 2 clouds
    cov_ms = kt_cov["knn_cov"]["avg_ms"] * kt_cov["knn_cov"]["count"] / 2
    k = 20
    rooflines = {
        "fdf_52B": roofline,
        "fdf_72B_read_rate": stored,
        "fdf_52B_c5_past_infinity_cache": c5_pass,
        "fdf_launched_52B": launched,
        "correspondence_plus_mahalanobis": roof(
            "vl_query_compact_kernel (listed 1-NN sweep with the Mahalanobis compaction fused, r04) + chunk_compact_list_kernel (its deferred chunks); once per outer iteration",
            CORR_BYTES, n_shard, corr_ms, kt["correspond"]["count"], "correspond_plus_compact",
            "SURVEY 8d: 72 B per source point (s 12 + Cs 24 + NN 12 + Ct 24)"),
        "knn_cov": roof(
            "knn_cov2_kernel<20> + knn_cov_kernel<20> hand-off (k-NN covariances, once per cloud per set_*)",
            COV_BYTES(k), args.n_target, cov_ms, 2, "knn_cov2_kernel",
            "SURVEY 8d: (k+1) x 12 + 24 = 276 B per point; time per cloud = both launches"),
    }
    kernels = {
        "knn_cov": kt_cov["knn_cov"],
        "correspond": kt["correspond"],
        "compact_mahalanobis": kt["compact"],
        "fdf": kt["fdf"],
        "reduce_finish": kt["reduce_finish"],
    }
    if not args.full:
        # no kernel-time or pass-bench leg ran: only the rows taken from the timed steps themselves hold figures
        rooflines = {k: rooflines[k] for k in ("fdf_52B", "fdf_72B_read_rate")}
        kernels = None

    fod = fod_rows(eng, scan, cad, T_final, args.fod_cpu_sample) if args.fod_cpu_sample > 0 and world == 1 else None
    cpu = None
    frob_sample = None
    full = None
    if args.cpu_sample > 0 and world == 1:  # the CPU baseline is an N=1 figure
        n_cpu = min(args.cpu_sample, args.n_source)
        rate, info, T_cpu, (s_scan, s_cad) = cpu_baseline(args, n_cpu, args.cpu_threads)
        scale = n_cpu / args.n_source
        single = {
            "value": rate * scale,
            "unit": "iterations/s",
            "cores": args.cpu_threads,
            "kind": "port",
            "sample": (f"oracle/gicp_ref.c (PCL 1.8.1 GICP restatement, kd-tree, BFGS) single align on a "
                       f"{n_cpu}<->{n_cpu} sample of the same synthetic workload: "
                       f"{info['iterations']} iterations in {info['t_loop_s']:.2f} s loop "
                       f"({rate:.3f} it/s at sample size; covariances {info['t_cov_s']:.2f} s), "
                       f"scaled x{scale:g} to {args.n_source} points (linear, favours the CPU)"),
            "sample_rate": rate,
            "sample_frac_scale": scale,
        }
        cpu = dict(single)
        # final-transform parity on the sample
        e3 = GICPEngine(device=local)
        e3.set_source_xyz(s_scan)
        e3.set_target_xyz(s_cad)
        T_gpu = e3.align()
        frob_sample = float(np.linalg.norm(T_gpu.astype(np.float64) - T_cpu.astype(np.float64)))
        if gn is not None:
            # GN mode against the oracle's GN restatement on the same sample
            from leica_point_cloud_processing_amd import _lib
            from oracle import ref

            og = ref.RefGICP(threads=max(1, args.cpu_threads), solver=1)
            og.set_source(s_scan)
            og.set_target(s_cad)
            T_ogn, _ = og.align()
            e3.setSolver(_lib.MGICP_SOLVER_GN)
            T_egn = e3.align()
            gn["frob_vs_oracle_gn_sample"] = float(np.linalg.norm(T_egn.astype(np.float64) - T_ogn.astype(np.float64)))
        e3.close()
        host = host_info()
        cpu["host"] = host
        if args.oracle_full:
            # the granted thread share (OMP_NUM_THREADS of the box's nproc), the FULL workload: the
            # stronger baseline (no scaling) and the full-size final-transform parity of the metric
            nt = host["threads_used"]
            T_o, oinfo = oracle_full(scan, cad, nt, args.max_iter, args.fixed)
            trace_err = (max(float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)))
                             for a, b in zip(trace_final, oinfo["trace"]))
                         if len(trace_final) == len(oinfo["trace"]) else None)
            all_rate = oinfo["iterations"] / oinfo["t_loop_s"]
            full = {
                "frob_vs_oracle": float(np.linalg.norm(T_final.astype(np.float64) - T_o.astype(np.float64))),
                "iterations_gpu": iters_per_align, "iterations_oracle": oinfo["iterations"],
                "converged_oracle": bool(oinfo["converged"]),
                "max_trace_frob_vs_oracle": trace_err,
                "oracle_threads": nt,
                "pinning": ("against the oracle's PCL 1.8.1 restatement (oracle/gicp_ref.c); UNPINNED against PCL "
                            "binaries: PCL is not in the image and the reference holds no output vector.  Flipping "
                            "one restated bfgs.h choice moves the C4 final T by 1.5-1.7e-2 (DESIGN.md 'Oracle "
                            "uncertainty ledger')"),
            }
            cpu = {
                "value": all_rate,
                "unit": "iterations/s",
                "cores": nt,
                "kind": "port",
                "sample": (f"oracle/gicp_ref.c with OpenMP on {nt} threads ({host['thread_share']}) over the FULL {args.n_source}<->"
                           f"{args.n_target} workload (no scaling): {oinfo['iterations']} iterations in "
                           f"{oinfo['t_loop_s']:.2f} s loop, covariances + kd-trees {oinfo['t_cov_s']:.2f} s, "
                           f"ms-to-converge {1e3 * oinfo['t_total_s']:.0f} ms"),
                "ms_to_converge": 1e3 * oinfo["t_total_s"],
                "host": host,
                "single_thread": single,
                "gpu_over_thread_share": value / all_rate,
                "gpu_over_single_thread": value / single["value"],
            }

    line = {
        "metric": ("GICP iterations/sec, 5M<->5M scan-vs-CAD (PCL-1.8.1-faithful BFGS GICP)" if args.config == "C4"
                   else f"GICP iterations/sec, {args.config} (PCL-1.8.1-faithful BFGS GICP)"),
        "value": round(value, 3),
        "unit": "iterations/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "full": bool(args.full),
        "ms_per_step": round(1e3 * dt / args.steps, 3),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32 transform / f64 accumulate",
        "data": "synthetic",
        "config": {
            "workload": f"{args.cfg_text} ({args.n_source} vs {args.n_target} points), synthetic aero part, "
                        f"k=20, maxCorrDist=0.04, tf_eps=4e-3, rot_eps=2e-3, max_iter={args.max_iter}, guess=I",
            "name": args.config,
            "n_source": args.n_source,
            "n_target": args.n_target,
            "parallelism": f"source point-range shards x{world}, target replicated",
            "transport": transport,
            "transport_notes": transport_notes,
        },
        "iterations_per_align": iters_per_align,
        "n_corr": result["n_corr"],
        "n_rejected_last_sweep": args.n_source - result["n_corr"] if world == 1 else None,
        "objective_passes_per_align": result["n_evals"],
        "vlist": vlist,
        "ms_to_converge_first": round(first["ms_total"], 3),
        "ms_create": round(ms_create, 3),
        "ms_create_parts": create_parts,
        "aligns_after_set": warm,
        # the cell lists' build time: the warmup aligns' wall time beyond the first list-free steady align
        "vlist_build_ms_estimate": (round(sum(max(0.0, a["ms_wall"] - warm[1]["ms_wall"]) for a in warm[2:]), 3)
                                    if len(warm) >= 3 else None),
        "ms_to_converge_new_clouds_warm_process": new_clouds,
        "ms_to_converge_first_detail": {k: round(first[k], 3) for k in ("ms_upload", "ms_prep", "ms_loop")},
        "ms_to_converge_cached": round(1e3 * dt / args.steps, 3),
        "cold_pair": cold_pair,
        "gicpstate_cycles": gicpstate,
        "frob_vs_oracle": full["frob_vs_oracle"] if full else None,
        "parity_full_size": full,
        "frob_vs_oracle_sample": frob_sample,
        "roofline": roofline,
        "rooflines": rooflines,
        "kernels": kernels,
        "cpu_baseline": cpu,
        "gn_mode": gn,
        "fod_rows": fod,
        "data_gen_s": round(t_gen, 2),
    }
    line["pass_stats_timed"] = pass_stats_timed
    eng.close()
    print(json.dumps(line))
    if pass_stats_timed["takeovers"] > 0:
        # a pass of the timed region missed its deadline and ran on the launched kernel: the number
        # above does not describe the resident path
        sys.stderr.write(f"bench.py: {pass_stats_timed['takeovers']} server take-over(s) in the timed region\n")
        sys.exit(3)


if __name__ == "__main__":
    main()
