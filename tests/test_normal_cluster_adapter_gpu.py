"""adapter/InitialAlignment_normals_mi355x.cpp -- obtainNormalsCluster and obtainDominantNormals over layout-exact
stand-ins (tests/adapter_standins_ia_normals), run in runNormalsBasedAlgorithm's order by the replay driver on a
3000-record scan of the synthetic part at quarter scale (at full scale its 3.4 cm spacing leaves the reference's
5 cm tolerance no cluster of 2.5 % of the records, and both sides only take the fallback): the clusters and the dominant normals it writes must hold the bytes the
Python mirror (initial_alignment.obtainNormalsCluster / obtainDominantNormals) gives for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _drive(args):
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_normals_cluster")
    assert os.path.exists(exe), "build it with `make normals-cluster-replay`"
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines())
              if len(p) == 2 and p[1] in ("ok", "FAIL")}
    assert checks and all(checks.values()), checks
    return checks


def test_the_two_members_equal_the_python_mirror(tmp_path):
    from leica_point_cloud_processing_amd import initial_alignment as ia
    from leica_point_cloud_processing_amd import synth
    from leica_point_cloud_processing_amd.engine import GICPEngine

    scan, _cad, _T = synth.scan_vs_cad(3000, 3000)
    xyz = np.ascontiguousarray(scan * np.float32(0.25), np.float32)
    with GICPEngine() as e:
        normals = np.ascontiguousarray(e.estimate_normals(xyz, 10.0 * e.cloud_resolution(xyz))[0][:, :3], np.float32)
        clusters = ia.obtainNormalsCluster(xyz, normals, e)
        dominant = ia.obtainDominantNormals(normals, clusters, e)
    assert len(xyz) == 3000 and len(clusters) >= 2 and len(clusters[0]) < 3000  # real clusters, not the fallback
    files = [tmp_path / f for f in ("cloud.bin", "normals.bin", "indices.bin", "sizes.bin", "dominant.bin")]
    xyz.tofile(files[0])
    normals.tofile(files[1])
    checks = _drive(files)
    assert len(checks) >= 7
    assert files[2].read_bytes() == np.concatenate(clusters).astype(np.int32).tobytes()
    assert files[3].read_bytes() == np.array([len(m) for m in clusters], np.int32).tobytes()
    assert files[4].read_bytes() == np.ascontiguousarray(dominant, np.float32).tobytes()
    print("part: clusters", [len(m) for m in clusters])
