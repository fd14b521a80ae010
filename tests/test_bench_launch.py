"""bench.py's own N > 1 launch: `python bench.py --gpus N` started WITHOUT
torchrun spawns N child ranks (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set by the parent), which
meet at the TCP rendezvous, share the shared-segment name and the RCCL id, and rank 0's JSON line is
relayed.  --dry-run stops before anything loads libmgicp.so, so this runs on the CPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2, 4])
def test_bench_spawns_its_own_ranks(n):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run"],
                         capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1  # only rank 0 prints
    rec = json.loads(lines[0])
    assert rec["dry_run"] and rec["n_gpus"] == n and rec["ranks_joined"] == n and rec["uid_ok"]
    assert rec["local_rank"] == 0 and rec["shm_name"].startswith("/mgicp_")


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) at a small size: --steps sets the timed steps, the line holds the headline
    fields and none of the --full legs, and --dump-outputs writes the last timed align's arrays."""
    import numpy as np

    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--n-source", "20000", "--n-target", "20000", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["full"] is False
    assert rec["unit"] == "iterations/s" and rec["higher_is_better"] is True and rec["value"] > 0
    assert rec["dtype"] == "f32 transform / f64 accumulate"
    assert rec["ms_per_step"] > 0
    # value = iterations of the timed steps / their seconds, ms_per_step = those seconds / steps (both
    # rounded to 3 decimals in the line)
    assert rec["value"] == pytest.approx(rec["iterations_per_align"] / (rec["ms_per_step"] * 1e-3), rel=5e-3)
    for leg in ("cpu_baseline", "gn_mode", "fod_rows", "cold_pair", "gicpstate_cycles", "parity_full_size",
                "ms_to_converge_new_clouds_warm_process", "kernels", "frob_vs_oracle", "frob_vs_oracle_sample"):
        assert rec[leg] is None, leg
    assert sorted(p.name for p in out_dir.iterdir()) == ["align_result.npy", "final_transformation.npy",
                                                         "iteration_transformations.npy"]
    T = np.load(out_dir / "final_transformation.npy")
    tr = np.load(out_dir / "iteration_transformations.npy")
    res = np.load(out_dir / "align_result.npy")
    assert T.dtype == np.float32 and T.shape == (4, 4) and np.isfinite(T).all()
    assert tuple(T[3]) == (0.0, 0.0, 0.0, 1.0)
    assert tr.dtype == np.float32 and tr.shape[1:] == (4, 4) and np.isfinite(tr).all()
    assert res.dtype == np.float64 and res.shape == (3,)
    assert res[1] == rec["iterations_per_align"] and res[2] == rec["n_corr"]
    assert len(tr) == rec["iterations_per_align"]
    np.testing.assert_array_equal(tr[-1], T)


def test_bench_legs_beyond_the_timed_steps_wait_for_full():
    """parse(): without --full every leg option is off whatever its own default; with --full they hold."""
    code = ("import sys, json, bench\n"
            "a = bench.parse()\n"
            "print(json.dumps([a.full, a.cpu_sample, a.fod_cpu_sample, a.oracle_full, a.gn_steps, a.pass_bench, "
            "a.cold_pairs, a.c5_leg, a.no_events, a.dump_outputs]))\n")
    got = {}
    for extra in ([], ["--full"], ["--full", "--gn-steps", "0", "--dump-outputs", "d"]):
        out = subprocess.run([sys.executable, "-c", code, "--gpus", "1", "--steps", "3", "--warmup", "1"] + extra,
                             capture_output=True, text=True, timeout=60, cwd=ROOT)
        assert out.returncode == 0, out.stderr
        got[len(extra)] = json.loads(out.stdout)
    assert got[0] == [False, 0, 0, 0, 0, 0, 0, 0, True, None]
    assert got[1] == [True, 500_000, 500_000, 1, 5, 5, 3, 1, False, None]
    assert got[5] == [True, 500_000, 500_000, 1, 0, 5, 3, 1, False, "d"]


def test_bench_launch_never_loads_the_engine_in_the_parent():
    """The parent of the spawned ranks must not load libmgicp.so (HIP) -- it only spawns and waits."""
    import ast

    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    fn = next(f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name == "launch_ranks")
    names = {n.id for n in ast.walk(fn) if isinstance(n, ast.Name)} | \
            {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute)}
    assert not names & {"GICPEngine", "_lib", "load", "execv", "execve", "execvp"}
    main = next(f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name == "main")
    first = main.body[:3]  # args, then the launch branch before any engine import
    assert any(isinstance(s, ast.If) and "launch_ranks" in ast.dump(s) for s in first)
