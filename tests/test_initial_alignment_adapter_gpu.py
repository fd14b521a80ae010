"""adapter/InitialAlignment_mi355x.cpp with its four members in ONE process, and so on the one engine context
the helper adapters share (adapter/EngineContext_mi355x.h): obtainBoundaryKeypoints, obtainHarrisKeypoints,
obtainFeatures on each keypoint set, obtainCorrespondences over the two feature clouds, then the first
member again.  Every file the combined driver writes must hold the bytes the single-member drivers -- a
process and a fresh context each -- write for the same inputs, and the repeated first call its first result.
"""
import os
import subprocess

import numpy as np
import pytest

import boundary_cases as bc
import harris_cases as hc
from conftest import ROOT

pytestmark = pytest.mark.gpu

FACTOR = 1.4  # the stand-in's radius_factor_, which replay_test_fpfh leaves at its default


def _drive(name, target, args):
    exe = os.path.join(ROOT, "adapter", "build", name)
    assert os.path.exists(exe), f"build it with `make {target}`"
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines())
              if len(p) == 2 and p[1] in ("ok", "FAIL")}
    assert checks and all(checks.values()), checks
    return checks


def test_four_members_on_one_context_equal_the_single_drivers(tmp_path):
    xyz_a, nrm_a, k = bc.case("part")  # the boundary adapter test's cloud
    assert k == 30
    xyz_b, nrm_b, _radius, _thr, _nonmax = hc.case("part_1p4")
    one, all4 = tmp_path / "single", tmp_path / "combined"
    one.mkdir()
    all4.mkdir()
    inputs = [tmp_path / f for f in ("cloud_a.bin", "normals_a.bin", "cloud_b.bin", "normals_b.bin")]
    for path, a in zip(inputs, (xyz_a, nrm_a, xyz_b, nrm_b)):
        np.ascontiguousarray(a, np.float32).tofile(path)

    checks = _drive("replay_test_initial_alignment", "ia-replay", inputs + [repr(FACTOR), all4])
    assert len(checks) >= 7

    _drive("replay_test_boundary", "boundary-replay", inputs[:2] + [one / "boundary_kp.bin", one / "boundary_nkp.bin"])
    _drive("replay_test_harris", "harris-replay", inputs[2:] + [repr(FACTOR), one / "harris_kp.bin"])
    _drive("replay_test_fpfh", "fpfh-replay", inputs[:2] + [one / "boundary_kp.bin", one / "fpfh_boundary.bin"])
    _drive("replay_test_fpfh", "fpfh-replay", inputs[2:] + [one / "harris_kp.bin", one / "fpfh_harris.bin"])
    _drive("replay_test_correspondences", "corr-replay",
           [one / "fpfh_boundary.bin", one / "fpfh_harris.bin"] +
           [one / f for f in ("corr_query.bin", "corr_match.bin", "corr_distance.bin")])

    names = ("boundary_kp.bin", "boundary_nkp.bin", "harris_kp.bin", "fpfh_boundary.bin", "fpfh_harris.bin",
             "corr_query.bin", "corr_match.bin", "corr_distance.bin")
    for f in names:
        got, want = (all4 / f).read_bytes(), (one / f).read_bytes()
        assert len(want) > 0, f  # the fixtures have keypoints of both kinds, features and correspondences
        assert got == want, f
    for f in ("boundary_kp.bin", "boundary_nkp.bin"):
        assert (all4 / f.replace("boundary_", "boundary_again_")).read_bytes() == (all4 / f).read_bytes(), f
