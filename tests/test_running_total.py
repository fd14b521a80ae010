"""The host's row total taken while the rows land (shm::RunningTotal, csrc/shm_rows.hpp) on the CPU: a
stand-alone program with its own main (tests/running_total_standalone/running_total_main.cpp) built with
g++ -- the header compiles without HIP -- plain and with AddressSanitizer + UBSan.

The program compares RunningTotal with shm::fixed_total by memcmp for nsup in {1, 2, 63, 64, 65, 127, 128,
129, 153, 192, 193} and 16 values per row, over rows chosen against a change of order or of the lanes'
starting value: magnitudes 1e-300 ... 1e300 mixed within one lane, cancelling pairs, -0.0 rows, denormals.
It prints one "<check> ok|FAIL" line per check (every check must be there and ok) and the time of one total
over 153 rows in both forms.
"""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "running_total_standalone", "running_total_main.cpp")
CSRC = os.path.join(ROOT, "leica_point_cloud_processing_amd", "csrc")
# -ffp-contract=off: the engine's host code is compiled that way (Makefile HIPFLAGS)
BASE = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]

CHECKS = {
    "uniform", "magnitudes", "cancelling_pairs", "negative_zero_rows", "zero_sign_mix", "denormals", "denormal_mix",
    "negative_zero_total_is_positive", "reuse_after_reset",
}


@pytest.mark.parametrize("flags", [["-O2"],
                                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_running_total_standalone(tmp_path, flags):
    exe = str(tmp_path / "running_total_main")
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
    assert "time of one total" in r.stdout
    assert not r.stderr.strip(), r.stderr  # a sanitizer report
