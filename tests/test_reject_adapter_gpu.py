"""adapter/InitialAlignment_transform_mi355x.cpp -- rejectCorrespondences, rejectOneToOneCorrespondences and
estimateTransform over layout-exact stand-ins (tests/adapter_standins_ia_transform), run in the order of
runKeypointsBasedAlgorithm by the replay driver: every file it writes must hold the bytes the engine's Python
calls give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

import reject_cases as rc
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _drive(args):
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_transform")
    assert os.path.exists(exe), "build it with `make transform-replay`"
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines())
              if len(p) == 2 and p[1] in ("ok", "FAIL")}
    assert checks and all(checks.values()), checks
    return checks


def test_the_three_members_equal_the_engine_calls(tmp_path):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    c = rc.case("clean_1000")
    rng = np.random.default_rng(5)
    # twenty pairs of good correspondences onto one target each (the second source point moved next to the
    # first), so that the one-to-one step has something to remove after the RANSAC step
    im, src = c.im.copy(), c.src.copy()
    good = np.flatnonzero(c.kind == 0)
    im[good[1:40:2]] = im[good[0:39:2]]
    src[c.iq[good[1:40:2]]] = src[c.iq[good[0:39:2]]] + np.float32(0.001)
    dist = rng.uniform(0, 50, len(c.iq)).astype(np.float32)
    c = rc._case(src, c.tgt, c.iq, im)
    inputs = [tmp_path / f for f in ("source_kp.bin", "target_kp.bin", "query.bin", "match.bin", "distance.bin")]
    for path, a in zip(inputs, (c.src, c.tgt, c.iq, im, dist)):
        np.ascontiguousarray(a).tofile(path)
    out = tmp_path / "out"
    out.mkdir()
    checks = _drive(inputs + [out])
    assert len(checks) >= 8

    with GICPEngine() as e:
        keep, _T, _info = e.reject_ransac(c.src, c.tgt, c.iq, im, 1.5, 1000, True)
        q1, m1, d1 = c.iq[keep], im[keep], dist[keep]
        T1, _ = e.estimate_rigid_svd(c.src, c.tgt, q1, m1)
        order, _ = e.reject_one_to_one(m1, d1, int(m1.max()) + 1)
        q2, m2, d2 = q1[order], m1[order], d1[order]
        T2, _ = e.estimate_rigid_svd(c.src, c.tgt, q2, m2)
    assert 3 <= len(q2) < len(q1) < len(c.iq)
    for name, want in (("ransac_query", q1), ("ransac_match", m1), ("ransac_distance", d1), ("one_query", q2),
                       ("one_match", m2), ("one_distance", d2), ("tf_ransac", T1.T), ("tf", T2.T)):
        assert (out / f"{name}.bin").read_bytes() == np.ascontiguousarray(want).tobytes(), name
