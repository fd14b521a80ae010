"""FODDetector::clusterPossibleFODs -> pcl::EuclideanClusterExtraction (src/FODDetector.cpp:45-58), the
last step of the inspection pipeline, on the engine (mgicp_euclidean_clusters, DESIGN.md "Euclidean
clustering").

The result is a partition fixed by one predicate on point pairs -- both finite and FLANN's float
((dx^2) + dy^2) + dz^2 < float(tolerance^2) -- so the bar is exact equality: clusters, their order
(size descending, ties by ascending smallest member), members ascending, labels and offsets.

Reference (tests/cluster_edges_cases.py, `ref_clusters`, shared with the cluster-edge tests): candidate
pairs from scipy's cKDTree at a slightly widened radius, filtered by the exact fp32 predicate (the numpy
float32 expression of tests/test_fod_filters.py `_bruteforce_keep`),
scipy.sparse.csgraph.connected_components, then the size filter and the ordering rule.  It is itself checked against an all-pairs brute force with its own
union-find.  PCL is not installed here: the order of equal-size clusters beyond 16 clusters is the
documented stable choice, not pinned against a PCL binary.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from cluster_edges_cases import bruteforce_clusters as _bruteforce_clusters
from cluster_edges_cases import components as _components
from cluster_edges_cases import finish as _finish
from cluster_edges_cases import fod_cloud as _fod_cloud
from cluster_edges_cases import r2_of as _r2
from cluster_edges_cases import ref_clusters as _ref_clusters
from conftest import ROOT
from leica_point_cloud_processing_amd.cloud import PointCloudRGB

FODREPLAY = os.path.join(ROOT, "adapter", "build", "replay_test_fod_detector")


def _cubes():
    """The three lattice cubes of test/test_fod_detector.cpp: fp32 loop counters from pos, += 0.1f."""
    out = []
    for pos in (0.0, 10.0, 20.0):
        axis, v, end = [], np.float32(pos), np.float32(pos) + np.float32(3.0)
        while v < end:
            axis.append(v)
            v = np.float32(v + np.float32(0.1))
        a = np.array(axis, np.float32)
        out.append(np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3))
    return np.concatenate(out).astype(np.float32)


# ---------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------
def test_reference_helper_matches_bruteforce():
    a = _fod_cloud(n=300)
    assert 380 <= len(a) <= 420
    for tol in (1e-30, 1e-4, 4e-3, 3e-2, 1.2):
        for mn, mx in ((1, 0), (3, 0), (1, 50)):
            rc, rl, ro, rn = _ref_clusters(a, tol, mn, mx)
            bc, bl, bo, bn = _bruteforce_clusters(a, tol, mn, mx)
            assert rn == bn and len(rc) == len(bc)
            for x, y in zip(rc, bc):
                np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(rl, bl)
            np.testing.assert_array_equal(ro, bo)
    # a non-trivial partition at the FOD threshold: several clusters, the non-finite records in none
    rc, rl, _, _ = _ref_clusters(a, 3e-2)
    assert len(rc) > 1 and rl[7] == -1 and rl[len(a) - 5] == -1


def test_reference_helper_known_figures():
    """The figures the other tests lean on, from the helper alone."""
    rc, _, _, _ = _ref_clusters(_cubes(), 0.12, 3)
    assert [len(c) for c in rc] == [29791, 27000, 27000]
    assert [int(c[0]) for c in rc] == [0, 29791, 56791]
    for xyz, want in _edge_cases():
        assert len(_ref_clusters(xyz, 0.5)[0]) == want
    x = (np.float32(0.009) * np.arange(5000, dtype=np.float32)).astype(np.float32)
    chain = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    assert [len(c) for c in _ref_clusters(chain, 0.01)[0]] == [5000]


def test_header_declares_and_lib_maps_the_symbol():
    from leica_point_cloud_processing_amd import _lib

    assert "mgicp_euclidean_clusters" in _lib.header_symbols()
    assert set(_lib.header_symbols()) == set(_lib._SIGNATURES)
    res, args = _lib._SIGNATURES["mgicp_euclidean_clusters"]
    assert res is ctypes.c_int and len(args) == 11
    # int, int, 5 doubles: the layout of mgicp_cluster_info in the header
    assert ctypes.sizeof(_lib.MgicpClusterInfo) == 48
    with open(_lib.HEADER_PATH) as f:
        assert "} mgicp_cluster_info;" in f.read()


def _make_fod_replay():
    r = subprocess.run(["make", "-s", "-C", ROOT, "fod-replay"], capture_output=True, text=True)
    assert r.returncode == 0, "make fod-replay failed:\n" + r.stdout + r.stderr
    assert os.path.exists(FODREPLAY), f"{FODREPLAY} missing after make fod-replay"
    return FODREPLAY


@pytest.fixture(scope="module")
def fod_replay():
    """The replay binary; built here (`make fod-replay`) when a GPU-only run finds none."""
    return FODREPLAY if os.path.exists(FODREPLAY) else _make_fod_replay()


def test_fod_adapter_compiles_against_standins():
    fod_replay = _make_fod_replay()
    nm = subprocess.run(["nm", "-C", fod_replay], capture_output=True, text=True).stdout
    assert "FODDetector::clusterPossibleFODs()" in nm
    assert "mgicp_euclidean_clusters" in nm


def test_fod_detector_arguments(caplog):
    from leica_point_cloud_processing_amd.fod_detector import FODDetector

    cloud = PointCloudRGB.from_xyz(np.zeros((4, 3), np.float32))
    with caplog.at_level("WARNING"):
        d = FODDetector(cloud, 0, 3.9)
    assert d.cluster_tolerance_ == 4e-3
    assert any("invalid tolerance" in r.getMessage() for r in caplog.records)
    assert d.min_cluster_size_ == 3.9 and d.minClusterSize() == 3  # the double is kept, PCL's int setter truncates
    d.setClusterTolerance(1.2)
    d.setMinFODpoints(7)
    assert d.cluster_tolerance_ == 1.2 and d.minClusterSize() == 7
    assert d.getFODIndices() == [] and d.fodIndicesToPointCloud() == (0, [])
    # values an int cannot hold: NaN and anything below 1 ask for every cluster, huge ones saturate
    for v, want in ((float("nan"), 0), (-5.0, 0), (0.5, 0), (1e30, 2147483647), (float("inf"), 2147483647)):
        d.setMinFODpoints(v)
        assert d.minClusterSize() == want, v
    assert d.cloud_ is cloud


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    e = GICPEngine()
    yield e
    e.close()


def _assert_same(got, ref):
    cl, lab, info = got
    rc, rl, ro, rn = ref
    assert [len(c) for c in cl] == [len(c) for c in rc]
    for x, y in zip(cl, rc):
        assert x.dtype == np.int32
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(lab, rl)
    np.testing.assert_array_equal(info["offsets"], ro)
    assert info["n_clusters"] == len(rc) and info["n_components"] == rn
    assert info["n_clustered_points"] == ro[-1]


def _check(eng, xyz, tol, mn=1, mx=0):
    got = eng.euclidean_clusters(xyz, tol, mn, mx)
    _assert_same(got, _ref_clusters(xyz, tol, mn, mx))
    return got


def _edge_cases():
    """(two points, expected clusters at tolerance 0.5): distance exactly 0.5 (d^2 == r^2: not linked)
    and one fp32 step closer, along each axis, at the origin and with both points offset by +1000 m."""
    out = []
    for off in (0.0, 1000.0):
        for ax in range(3):
            far = np.float32(off + 0.5)
            for second, want in ((far, 2), (np.nextafter(far, np.float32(0)), 1)):
                p = np.full((2, 3), off, np.float32)
                p[1, ax] = second
                out.append((p, want))
    return out


@pytest.mark.gpu
def test_threshold_edge(eng):
    for xyz, want in _edge_cases():
        cl, _, _ = _check(eng, xyz, 0.5)
        assert len(cl) == want, xyz
    # float(tolerance^2) == 0 links nothing, not even the duplicate pair
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, (10, 3)).astype(np.float32)
    p[6] = p[2]
    cl, lab, info = _check(eng, p, 1e-30)
    assert [len(c) for c in cl] == [1] * 10 and info["pair_tests"] == 0
    np.testing.assert_array_equal(lab, np.arange(10))


def _chain(gap_at=None):
    x = (np.float32(0.009) * np.arange(5000, dtype=np.float32)).astype(np.float32)
    if gap_at is not None:
        # widen one gap to the tolerance at fp32 granularity: the smallest next coordinate whose float
        # difference d has float d*d >= float(tol^2) (one step closer still links)
        r2, a = _r2(0.01), x[gap_at]
        b = np.float32(a + np.float32(0.0099))
        while np.float32(np.float32(b - a) * np.float32(b - a)) < r2:
            b = np.nextafter(b, np.float32(np.inf))
        prev = np.nextafter(b, np.float32(0))
        assert np.float32(np.float32(prev - a) * np.float32(prev - a)) < r2
        x[gap_at + 1:] = (b + np.float32(0.009) * np.arange(5000 - gap_at - 1, dtype=np.float32)).astype(np.float32)
    perm = np.random.default_rng(11).permutation(5000)
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)[perm], perm


@pytest.mark.gpu
def test_long_chain(eng):
    xyz, _ = _chain()
    cl, lab, _ = _check(eng, xyz, 0.01)
    assert len(cl) == 1
    np.testing.assert_array_equal(cl[0], np.arange(5000))
    xyz, perm = _chain(gap_at=2500)
    cl, lab, _ = _check(eng, xyz, 0.01)
    assert sorted(len(c) for c in cl) == [2499, 2501]
    # the side of the gap decides the cluster
    np.testing.assert_array_equal(lab[np.argsort(perm)][:2501], np.full(2501, lab[np.argsort(perm)][0]))


@functools.lru_cache(maxsize=None)
def _fod_components(tol):
    return _components(_fod_cloud(), tol)


@pytest.mark.gpu
@pytest.mark.parametrize("mn,mx", [(1, 0), (3, 0), (1, 50)])
@pytest.mark.parametrize("tol", [1e-4, 4e-3, 3e-2, 1.2])
def test_random_part(eng, tol, mn, mx):
    a = _fod_cloud()
    fin_idx, comp = _fod_components(tol)
    got = eng.euclidean_clusters(a, tol, mn, mx)
    _assert_same(got, _finish(a, fin_idx, comp, mn, mx))
    assert got[1][7] == -1 and got[1][len(a) - 5] == -1  # the NaN and the Inf record
    # the same through the 32-byte PointXYZRGB records
    got = eng.euclidean_clusters(PointCloudRGB.from_xyz(a), tol, mn, mx)
    _assert_same(got, _finish(a, fin_idx, comp, mn, mx))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_at_wave_and_block_edges(eng, n):
    from scipy.spatial import cKDTree

    p = np.random.default_rng(n).uniform(0, 1, (n, 3)).astype(np.float32)
    tol = 0.1
    if n > 1:  # the median nearest-neighbour distance: about half the points link to their neighbour
        tol = float(np.median(cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=2)[0][:, 1]))
    cl, _, info = _check(eng, p, tol)
    if n > 64:
        assert 1 < len(cl) < n


@pytest.mark.gpu
def test_reference_replay_python():
    from leica_point_cloud_processing_amd.fod_detector import FODDetector

    cloud = PointCloudRGB.from_xyz(_cubes(), rgb=0x00ffffff)
    assert cloud.size() == 83791
    d = FODDetector(cloud, 4e-3 * 3 * 10, 3)
    d.clusterPossibleFODs()
    idx = d.getFODIndices()
    assert [len(c) for c in idx] == [29791, 27000, 27000]
    assert [int(c[0]) for c in idx] == [0, 29791, 56791]
    n, clouds = d.fodIndicesToPointCloud()
    assert n == 3 and len(clouds) == 3
    for c, i in zip(clouds, idx):
        assert np.all(np.diff(i) > 0)
        np.testing.assert_array_equal(c.points, cloud.points[i])
    # testEmptyCloud
    e = FODDetector(PointCloudRGB(), 4e-3 * 3 * 10, 3)
    e.clusterPossibleFODs()
    assert e.fodIndicesToPointCloud() == (0, [])


@pytest.mark.gpu
def test_reference_replay_adapter(fod_replay):
    r = subprocess.run([fod_replay], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    checks = {p[0]: p[1] == "ok" for p in (ln.split() for ln in r.stdout.splitlines())
              if len(p) == 2 and p[1] in ("ok", "FAIL")}
    assert set(checks) == {"testFODClustering_count", "testFODClustering_clouds", "testFODClustering_ascending",
                           "testFODClustering_copies", "testEmptyCloud_count", "testEmptyCloud_clouds",
                           "no_error_logged"}
    assert all(checks.values()), checks
    assert "points 83791" in r.stdout
    for line in ("cluster 0 size 29791 first 0", "cluster 1 size 27000 first 29791",
                 "cluster 2 size 27000 first 56791"):
        assert line in r.stdout, r.stdout


@pytest.mark.gpu
def test_tie_order(eng):
    rng = np.random.default_rng(5)
    centres = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    assert len(centres) == 40
    pts = (centres[:, None, :] + rng.uniform(-0.01, 0.01, (40, 3, 3))).reshape(-1, 3).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    cl, _, _ = _check(eng, pts, 0.05)
    assert [len(c) for c in cl] == [3] * 40  # more than 16 equal-size clusters
    firsts = [int(c[0]) for c in cl]
    assert firsts == sorted(firsts)


@pytest.mark.gpu
def test_dense_ball_uses_the_same_cell_shortcut(eng):
    rng = np.random.default_rng(9)
    a = rng.uniform(0, 0.2, (50000, 3))
    b = rng.uniform(0, 0.05, (500, 3)) + np.array([5.0, 0, 0])
    pts = np.concatenate([a, b]).astype(np.float32)
    perm = rng.permutation(len(pts))
    pts = pts[perm]
    cl, lab, info = eng.euclidean_clusters(pts, 1.2)
    assert len(cl) == 2 and info["n_components"] == 2
    np.testing.assert_array_equal(cl[0], np.flatnonzero(perm < 50000))
    np.testing.assert_array_equal(cl[1], np.flatnonzero(perm >= 50000))
    np.testing.assert_array_equal(lab, (perm >= 50000).astype(np.int32))
    n = len(pts)
    print("dense ball pair_tests", info["pair_tests"], "all pairs", n * (n - 1) // 2)
    assert info["pair_tests"] <= n * (n - 1) / 2 / 10
    # the same ball stretched over several cells of tol / 2 per axis: the cells are joined by the first
    # link found between each pair of them, still far from all pairs
    pts[:, :] = np.where((perm < 50000)[:, None], pts * np.float32(7.0), pts)
    cl, lab, info = eng.euclidean_clusters(pts, 1.2)
    assert len(cl) == 2
    np.testing.assert_array_equal(lab, (perm >= 50000).astype(np.int32))
    print("stretched ball pair_tests", info["pair_tests"])
    assert 0 < info["pair_tests"] <= n * (n - 1) / 2 / 10


@pytest.mark.gpu
def test_capped_grid_regime(eng):
    rng = np.random.default_rng(13)
    # two 300-point clumps 2 km apart along x at tolerance 1e-3: cells of tol / 2 would be 4e6 x 20 x 20
    clump = rng.uniform(0, 0.01, (2, 300, 3))
    clump[1, :, 0] += 2000.0
    pts = clump.reshape(-1, 3).astype(np.float32)
    cl, _, info = _check(eng, pts, 1e-3)
    assert 2 < len(cl) < 600
    # clumps at the corners of a 20 m box: 4e4 cells of tol / 2 per axis, the dense table's cap grows them
    corners = np.array([[0, 0, 0], [20, 20, 0], [20, 0, 20], [0, 20, 20]], np.float64)
    pts = (corners[:, None, :] + rng.uniform(0, 0.01, (4, 150, 3))).reshape(-1, 3).astype(np.float32)
    cl, _, _ = _check(eng, pts, 1e-3)
    assert 4 < len(cl) < 600


@pytest.mark.gpu
def test_invalid_and_empty(eng):
    from leica_point_cloud_processing_amd import _lib

    p = np.zeros((3, 3), np.float32)
    for tol in (-1.0, float("nan")):
        with pytest.raises(_lib.MgicpError) as ei:
            eng.euclidean_clusters(p, tol)
        assert ei.value.code == _lib.MGICP_E_INVALID
    for mn, mx in ((-1, 0), (1, -3)):  # would wrap to a huge size_t: refused before the call
        with pytest.raises(ValueError):
            eng.euclidean_clusters(p, 0.1, mn, mx)
    cl, lab, info = eng.euclidean_clusters(np.zeros((0, 3), np.float32), 0.1)
    assert cl == [] and len(lab) == 0 and info["n_clusters"] == 0 and info["n_components"] == 0
    # every record non-finite: no component at all
    cl, lab, info = eng.euclidean_clusters(np.full((5, 3), np.nan, np.float32), 0.1)
    assert cl == [] and list(lab) == [-1] * 5 and info["n_components"] == 0
    # three coincident points: one cluster
    cl, _, _ = _check(eng, p, 0.1)
    assert [len(c) for c in cl] == [3]


@pytest.mark.gpu
def test_state_isolation(part_small):
    """Clustering uses the helper cloud slot: a set source / target and their cached state stay."""
    from leica_point_cloud_processing_amd.engine import GICPEngine

    scan, cad, _ = part_small
    blobs = _fod_cloud()
    e = GICPEngine()
    try:
        e.set_source_xyz(scan)
        e.set_target_xyz(cad)
        T1 = e.align().copy()
        c1 = e.euclidean_clusters(blobs, 3e-2, 3)
        e.segment_differences(blobs, cad, 1.2e-2)
        c2 = e.euclidean_clusters(blobs, 3e-2, 3)
        T2 = e.align().copy()
    finally:
        e.close()
    assert T1.tobytes() == T2.tobytes()
    assert len(c1[0]) == len(c2[0]) > 1
    for x, y in zip(c1[0], c2[0]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(c1[1], c2[1])
    _assert_same(c1, _ref_clusters(blobs, 3e-2, 3))
