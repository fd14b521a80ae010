"""The per-run table of evaluated transforms (csrc/pass_memo.hpp) on the CPU: a stand-alone program with
its own main (tests/pass_memo_standalone/pass_memo_main.cpp) built with g++ -- the header and
csrc/pcl_bfgs.hpp compile without HIP -- plain and with AddressSanitizer + UBSan.

The program runs PclBfgs over a stub functor with the device functor's structure (sums of a pass depend on
the state only through its fp32 transform; f and g come from the sums and the doubles of the state), four
chained runs with the table and four without, and checks the table itself (full, the sign of a zero,
non-finite keys).  It prints one "<check> ok|FAIL" line per check; every check must be there and ok.
"""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "pass_memo_standalone", "pass_memo_main.cpp")
CSRC = os.path.join(ROOT, "leica_point_cloud_processing_amd", "csrc")
# -ffp-contract=off: the engine's host code is compiled that way (Makefile HIPFLAGS)
BASE = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]

CHECKS = {
    "table_fills_to_capacity", "table_full_stops_inserting", "table_full_keeps_every_entry",
    "table_zero_sign_is_a_miss", "table_zero_signs_are_two_keys", "table_refuses_non_finite_keys",
    "table_takes_the_finite_key", "table_non_finite_lookup_misses",
    "solver_evaluations_bitwise_equal", "solver_final_x_bitwise_equal", "solver_fewer_passes_with_table",
    "solver_hits_plus_passes_equal_untabled_passes", "solver_no_hits_without_table",
}


@pytest.mark.parametrize("flags", [["-O2"],
                                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_pass_memo_standalone(tmp_path, flags):
    exe = str(tmp_path / "pass_memo_main")
    r = subprocess.run(BASE + flags + ["-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    checks = {}
    for line in r.stdout.splitlines():
        parts = line.split()
        if len(parts) == 2 and parts[1] in ("ok", "FAIL"):
            checks[parts[0]] = parts[1] == "ok"
    assert set(checks) == CHECKS, set(checks) ^ CHECKS
    assert all(checks.values()), checks
    assert not r.stderr.strip(), r.stderr  # a sanitizer report
