"""the FOD-side callers either side of the GICP path.

  * Filter::removeFromCloud -> pcl::SegmentDifferences (src/Filter.cpp:176-189, called at
    src/LeicaStateMachine.cpp:187 with threshold 4e-3 * voxelize_factor on the cloud
    transformed at :182);
  * Filter::downsampleCloud -> pcl::VoxelGrid<PointXYZRGB> (src/Filter.cpp:91-105).

Oracle: oracle/gicp_ref.c ref_segment_differences / ref_voxel_grid (PCL 1.8.1 restatements),
themselves checked here against brute-force numpy.  Bars: keep masks and voxel sets bit-exact;
centroid xyz and colour bit-exact against the oracle (both sum each leaf in input order); the
reference's own tests hold no fixture for either filter -> pinned by brute force and by PCL's
published algorithm only.
"""
import numpy as np
import pytest

from leica_point_cloud_processing_amd.cloud import PointCloudRGB


def _bruteforce_keep(a, b, thr):
    keep = np.zeros(len(a), bool)
    fin_b = b[np.isfinite(b).all(1)]
    for i in range(len(a)):
        if not np.isfinite(a[i]).all():
            continue
        if len(fin_b) == 0:
            continue
        d = fin_b - a[i]
        d2 = ((d[:, 0] * d[:, 0]).astype(np.float32) + (d[:, 1] * d[:, 1]).astype(np.float32)).astype(np.float32)
        d2 = (d2 + (d[:, 2] * d[:, 2]).astype(np.float32)).astype(np.float32)
        keep[i] = np.float64(d2.min()) > thr
    return keep


def _fod_case(seed=0, n=3000, nsub=2500):
    """CAD-like target and a scan with a few foreign-object blobs (the FOD scenario)."""
    from leica_point_cloud_processing_amd import synth

    scan, cad, _ = synth.scan_vs_cad(n, nsub)
    rng = np.random.default_rng(seed)
    blobs = (cad[rng.integers(0, len(cad), 4)][:, None, :] +
             rng.normal(0, 0.004, (4, 25, 3)) + np.array([0, 0, 0.03])).reshape(-1, 3).astype(np.float32)
    return np.concatenate([scan, blobs]).astype(np.float32), cad


def test_oracle_segment_differences_matches_bruteforce():
    from oracle import ref

    a, b = _fod_case(n=1500, nsub=1200)
    a[7] = np.nan
    b[3] = np.inf
    for thr in (0.0, 1e-5, 1.2e-2 ** 2, 1.2e-2):
        keep, cnt = ref.segment_differences(a, b, thr)
        np.testing.assert_array_equal(keep, _bruteforce_keep(a, b, thr))
        assert cnt == keep.sum()
    keep, cnt = ref.segment_differences(a, np.zeros((0, 3), np.float32), 1.0)
    assert keep.all() and cnt == len(a)  # empty target: input - {} = input


def _bruteforce_voxels(rec, leaf, min_points=0):
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)
    fin = np.isfinite(xyz).all(1)
    inv = (np.float32(1.0) / np.asarray(leaf, np.float32)).astype(np.float32)  # one leaf or one per axis
    mn, mx = xyz[fin].min(0), xyz[fin].max(0)
    min_b = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(xyz[fin] * inv) - min_b.astype(np.float32)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    src = np.nonzero(fin)[0]
    order = np.lexsort((src, idx))
    out, cols = [], []
    for v in np.unique(idx):
        members = src[order][idx[order] == v]
        if len(members) < min_points:
            continue
        s = np.zeros(3, np.float32)
        for j in members:
            s = (s + xyz[j]).astype(np.float32)
        out.append((s / np.float32(len(members))).astype(np.float32))
        c = rec["rgb"][members].astype(np.uint32)
        ch = [np.float32(0)] * 4
        for cc in c:
            ch = [np.float32(ch[0] + np.float32(cc & 0xff)), np.float32(ch[1] + np.float32((cc >> 8) & 0xff)),
                  np.float32(ch[2] + np.float32((cc >> 16) & 0xff)), np.float32(ch[3] + np.float32(cc >> 24))]
        k = np.float32(len(members))
        cols.append((int(ch[3] / k) << 24) | (int(ch[2] / k) << 16) | (int(ch[1] / k) << 8) | int(ch[0] / k))
    return np.array(out, np.float32).reshape(-1, 3), np.array(cols, np.uint32)


def _rgb_cloud(n=4000, seed=1):
    from leica_point_cloud_processing_amd import synth

    scan, _, _ = synth.scan_vs_cad(n, 100)
    c = PointCloudRGB.from_xyz(scan)
    rng = np.random.default_rng(seed)
    c.points["rgb"] = rng.integers(0, 2 ** 32, len(scan), dtype=np.uint64).astype(np.uint32)
    return c


def test_oracle_voxel_grid_matches_bruteforce():
    from oracle import ref

    c = _rgb_cloud(3000)
    c.points["x"][5] = np.nan
    for leaf, mp in ((0.012, 0), (0.05, 0), (0.05, 3)):
        xyz, rgba, ovf = ref.voxel_grid(c.points, leaf, mp)
        bx, bc = _bruteforce_voxels(c.points, leaf, mp)
        assert not ovf
        np.testing.assert_array_equal(xyz, bx)
        np.testing.assert_array_equal(rgba, bc)


def test_oracle_voxel_grid_overflow_returns_input():
    from oracle import ref

    c = _rgb_cloud(200)
    c.points["x"][0] = 1e6  # a far outlier: 2^31 leaves at 1 mm
    xyz, rgba, ovf = ref.voxel_grid(c.points, 1e-3)
    assert ovf and len(xyz) == 200
    np.testing.assert_array_equal(rgba, c.points["rgb"])


# ---------------------------------------------------------------------------------------
# GPU parity
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    e = GICPEngine()
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.0, 1e-5, 1.2e-2 ** 2, 1.2e-2])
def test_segment_differences_gpu_matches_oracle(eng, thr):
    from oracle import ref

    a, b = _fod_case(n=20000, nsub=20000)
    a[11] = np.nan
    b[5] = np.nan  # KdTreeFLANN drops non-finite target points
    keep_ref, cnt_ref = ref.segment_differences(a, b, thr)
    keep, cnt = eng.segment_differences(a, b, thr)
    np.testing.assert_array_equal(keep, keep_ref)
    assert cnt == cnt_ref


@pytest.mark.gpu
def test_segment_differences_gpu_transform_and_edges(eng):
    """The FSM's transformPointCloud (LeicaStateMachine.cpp:182) fused as T; empty and
    all-non-finite targets; lattice ties at exactly the threshold distance."""
    from oracle import ref

    a, b = _fod_case(n=5000, nsub=5000)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.01, -0.004, 0.002]
    moved = (a.astype(np.float32) @ T[:3, :3].T.astype(np.float32) + T[:3, 3]).astype(np.float32)
    keep_ref, _ = ref.segment_differences(moved, b, 1.2e-2)
    keep, _ = eng.segment_differences(a, b, 1.2e-2, T=T)
    np.testing.assert_array_equal(keep, keep_ref)
    keep, cnt = eng.segment_differences(a, np.zeros((0, 3), np.float32), 1.0)
    assert keep.all() and cnt == len(a)
    keep, cnt = eng.segment_differences(a, np.full((10, 3), np.nan, np.float32), 1.0)
    assert not keep.any() and cnt == 0
    # integer lattice: d2 = exactly the threshold must NOT be kept (PCL: d2 > threshold)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    lat = (g * 0.25).astype(np.float32)
    q = lat + np.float32(0.25) * np.array([1, 0, 0], np.float32)
    keep, _ = eng.segment_differences(q, lat, 0.0625)
    keep_ref, _ = ref.segment_differences(q, lat, 0.0625)
    np.testing.assert_array_equal(keep, keep_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("leaf,mp", [(0.004, 0), (0.012, 0), (0.05, 0), (0.05, 4)])
def test_voxel_grid_gpu_matches_oracle(eng, leaf, mp):
    from oracle import ref

    c = _rgb_cloud(50000)
    c.points["y"][17] = np.inf
    xyz_ref, rgba_ref, _ = ref.voxel_grid(c.points, leaf, mp)
    out = eng.voxel_grid(c, leaf, mp)
    assert len(out) == len(xyz_ref)
    np.testing.assert_array_equal(out.xyz(), xyz_ref)
    np.testing.assert_array_equal(out.points["rgb"], rgba_ref)
    assert np.all(out.points["w"] == 1.0)


@pytest.mark.gpu
def test_voxel_grid_gpu_overflow_and_filter_class(eng):
    from leica_point_cloud_processing_amd.filter import Filter

    c = _rgb_cloud(300)
    c.points["x"][0] = 1e6
    out = eng.voxel_grid(c, 1e-3)
    assert len(out) == 300
    np.testing.assert_array_equal(out.points["rgb"], c.points["rgb"])
    # Filter::downsampleCloud / removeFromCloud drive the same kernels
    c = _rgb_cloud(20000)
    f = Filter(0.1)
    d = PointCloudRGB()
    f.downsampleCloud(c, d)
    assert 0 < len(d) < len(c)
    sub = PointCloudRGB()
    Filter.removeFromCloud(c, d, 1e-4, sub)
    assert 0 < len(sub) < len(c)


# ---------------------------------------------------------------------------------------
# The reference's own Filter tests (test/test_filter.cpp), same data, same assertions
# ---------------------------------------------------------------------------------------
def _filter_fixture_clouds():
    """gtest runs TestFilter's cases in file order, each constructing the fixture (one
    5000-point cube, 15000 rand() calls) from the shared glibc rand() stream (default seed):
    testDownsample sees calls 0..14999, testBox 15000..29999, testDifference 30000..44999 plus
    its own target cube (x = 2) from 45000..59999."""
    from leica_point_cloud_processing_amd import synth

    rng = synth.GlibcRand(1)
    down = synth.filter_test_cube(rng)
    synth.filter_test_cube(rng)  # testBox's fixture
    diff_src = synth.filter_test_cube(rng)
    diff_tgt = synth.filter_test_cube(rng, x=2.0)
    return down, diff_src, diff_tgt


def _white(xyz):
    c = PointCloudRGB.from_xyz(xyz)
    c.points["rgb"] = 0xFFFFFFFF  # r = g = b = 255 (alpha 255)
    return c


def test_filter_fixture_reproduction():
    down, diff_src, diff_tgt = _filter_fixture_clouds()
    assert down.shape == (5000, 3) and (down >= 0).all() and (down <= 5).all()
    assert (diff_tgt >= 2).all() and (diff_tgt <= 7).all()
    # the first glibc rand() after srand(1) is 1804289383
    assert down[0, 0] == np.float32(5.0 * 1804289383 / 2147483647.0)


@pytest.mark.gpu
def test_reference_testDownsample(eng):
    """test_filter.cpp:63-77: leaf = 2 * computeCloudResolution; the downsampled cloud's
    resolution is larger.  Also bit-exact against the VoxelGrid restatement."""
    from leica_point_cloud_processing_amd.filter import Filter
    from oracle import ref

    down, _, _ = _filter_fixture_clouds()
    cloud = _white(down)
    res = eng.cloud_resolution(cloud)
    leaf = float(np.float32(2 * res))
    out = PointCloudRGB()
    Filter(leaf).downsampleCloud(cloud, out)
    assert eng.cloud_resolution(out) > res
    xyz_ref, rgba_ref, _ = ref.voxel_grid(cloud.points, leaf)
    np.testing.assert_array_equal(out.xyz(), xyz_ref)
    np.testing.assert_array_equal(out.points["rgb"], rgba_ref)


@pytest.mark.gpu
def test_reference_testDifference(eng):
    """test_filter.cpp:95-106: removeFromCloud(target, source, res, diff) leaves a valid
    (size > 1) cloud.  Also bit-exact against the SegmentDifferences restatement."""
    from leica_point_cloud_processing_amd.filter import Filter
    from oracle import ref

    _, src, tgt = _filter_fixture_clouds()
    source, target = _white(src), _white(tgt)
    res = eng.cloud_resolution(source)
    diff = PointCloudRGB()
    Filter.removeFromCloud(target, source, res, diff)
    assert len(diff) > 1  # Utils::isValidCloud
    keep_ref, cnt_ref = ref.segment_differences(tgt, src, res)
    assert len(diff) == cnt_ref
    np.testing.assert_array_equal(diff.xyz(), tgt[keep_ref])


def _utils_lattice(dim=3.0, step=0.1):
    """TestUtils::cubeXYZ / cubeRGB (test_utils.cpp:31-60): float loop counters i += step."""
    vals = []
    v = np.float32(0.0)
    while v < np.float32(dim):
        vals.append(v)
        v = np.float32(v + np.float32(step))
    g = np.array(vals, np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.float32)


@pytest.mark.gpu
def test_reference_testCloudResolution(eng):
    """test_utils.cpp:77-91: the resolution of a 0.1-step lattice is within
    0.05 of 0.1, for PointXYZ (16-byte records) and PointXYZRGB (32-byte records) alike; the GPU
    2-NN mean equals a brute-force numpy evaluation."""
    from leica_point_cloud_processing_amd.cloud import PointCloudRGB as RGB

    import ctypes

    xyz = _utils_lattice()
    rec16 = np.zeros((len(xyz), 4), np.float32)  # pcl::PointXYZ records (x, y, z, pad)
    rec16[:, :3] = xyz
    rec16[:, 3] = 1.0
    out = ctypes.c_double()
    rc = eng._lib.mgicp_cloud_resolution(eng._h, ctypes.c_void_p(rec16.ctypes.data), len(rec16), 16,
                                         ctypes.byref(out))
    assert rc == 0
    res_xyz = out.value
    res_rgb = eng.cloud_resolution(RGB.from_xyz(xyz, rgb=0xFFFFFFFF))
    assert 0.05 <= res_xyz <= 0.15 and 0.05 <= res_rgb <= 0.15
    assert res_xyz == res_rgb
    # brute force on a sub-lattice corner (same float arithmetic: fp32 d2, sqrt in fp32, fp64 mean)
    sub = xyz[(xyz < np.float32(0.55)).all(1)]
    d = sub[:, None, :] - sub[None, :, :]
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + d[..., 2] * d[..., 2]).astype(np.float32)
    np.fill_diagonal(d2, np.inf)
    expect = float(np.mean(np.sqrt(d2.min(1)).astype(np.float64)))
    assert abs(eng.cloud_resolution(sub) - expect) <= 1e-12
