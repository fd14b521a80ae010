"""mgicp_normal_clusters and mgicp_dominant_normals (InitialAlignment::obtainNormalsCluster, obtainDominantNormals)
on the GPU against the NumPy reference of tests/normal_cluster_cases.py, whose decisions
test_normal_cluster_inputs.py shows to be firm.

Labels, indices and offsets must equal the reference's exactly, at every value of the "nc_small_limit" debug
option a case names (0: the default, 1: every multi-record round leaves the one-workgroup path, and for the long
rounds a limit one below, at and one above the round's size), and three calls must give the same bits.  The
dominant normals must equal the float64 restatement of the header's tree bit for bit.
"""
import ctypes

import numpy as np
import pytest

import normal_cluster_cases as nc

pytestmark = pytest.mark.gpu

_ENGINE = []


def _engine():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    if not _ENGINE:
        _ENGINE.append(GICPEngine())
    return _ENGINE[0]


def _call(e, c, limit=0, **over):
    e.debug_option("nc_small_limit", limit)
    try:
        a = dict(tol=c.tol, eps_angle=c.eps_angle, min_size=c.min_size, max_size=c.max_size)
        a.update(over)
        return e.normal_clusters(c.xyz, c.normals, a["tol"], a["eps_angle"], a["min_size"], a["max_size"])
    finally:
        e.debug_option("nc_small_limit", 0)


def _assert_equal(got, ref, what):
    clusters, labels, info = got
    assert labels.tobytes() == ref.labels.tobytes(), what
    assert info["offsets"].tolist() == ref.offsets.tolist(), what
    assert len(clusters) == len(ref.clusters), what
    got_idx = np.concatenate(clusters) if clusters else np.zeros(0, np.int32)
    assert got_idx.tobytes() == ref.indices.tobytes(), what
    assert info["n_rounds"] == ref.n_rounds and info["n_clusters"] == len(ref.clusters), what
    assert info["n_clustered_points"] == len(ref.indices), what


@pytest.mark.parametrize("name", nc.CASES)
def test_clusters_equal_the_reference_at_every_limit_and_on_every_call(name):
    e, c, ref = _engine(), nc.case(name), nc.case_reference(name)
    for limit in c.limits:
        first = None
        for call in range(3):
            got = _call(e, c, limit)
            _assert_equal(got, ref, (name, limit, call))
            bits = (got[1].tobytes(), got[2]["offsets"].tobytes(), b"".join(m.tobytes() for m in got[0]),
                    got[2]["pair_tests"], got[2]["n_levels"], got[2]["n_wide_rounds"])
            first = first or bits
            assert bits == first, (name, limit, call)


def test_the_small_limit_decides_where_a_round_runs_and_nothing_else():
    e = _engine()
    for name in ("long_line", "plane"):
        c = nc.case(name)
        size = len(c.xyz)
        wide = {limit: _call(e, c, limit)[2] for limit in c.limits}
        assert wide[1]["n_wide_rounds"] == 1 and wide[1]["n_levels"] >= 1
        # the round passes size - 1 at its last productive level: handed over with that frontier, one launch
        assert wide[size - 1]["n_wide_rounds"] == 1 and wide[size - 1]["n_levels"] == 1
        assert wide[size]["n_wide_rounds"] == 0 and wide[size + 1]["n_wide_rounds"] == 0
        assert wide[size]["n_levels"] == 0
        assert len({i["pair_tests"] for i in wide.values()}) == 1
    line = _call(e, nc.case("long_line"), 1)[2]
    assert line["n_levels"] == 299  # the seed's level runs in the workgroup, the 299 after it are launches


def test_a_level_larger_than_the_lds_frontier_is_handed_over_whole():
    """the blob's first level claims 4199 records, 103 more than the LDS frontier holds: at a limit of 4096 the
    round leaves the workgroup with the spilled frontier, whose one launch finds nothing more"""
    info = _call(_engine(), nc.case("blob"), 4096)[2]
    assert info["n_rounds"] == 1 and info["n_wide_rounds"] == 1 and info["n_levels"] == 1


def test_many_rounds_are_counted_exactly():
    info = _call(_engine(), nc.case("lattice"))[2]
    assert info["n_rounds"] == 4096 and info["n_clusters"] == 4096 and info["n_wide_rounds"] == 0
    print("lattice: n_levels", info["n_levels"], "pair_tests", info["pair_tests"], "ms_device", info["ms_device"])


def test_trivial_arguments():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    clusters, labels, info = e.normal_clusters(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), nc.TOL, nc.EPS)
    assert clusters == [] and len(labels) == 0 and info["n_rounds"] == 0
    clusters, labels, info = e.normal_clusters(np.zeros((1, 3), np.float32), np.float32([[0, 0, 1]]), nc.TOL, nc.EPS)
    assert [m.tolist() for m in clusters] == [[0]] and labels.tolist() == [0] and info["n_rounds"] == 1
    c = nc.case("patch_unit")
    # tolerance 0 links nothing, not even the record itself: singletons
    got = _call(e, c, tol=0.0)
    assert [m.tolist() for m in got[0]] == [[i] for i in range(100)]
    # max_size below the largest cluster: it is consumed and not reported
    got = _call(e, c, max_size=99)
    assert got[0] == [] and np.all(got[1] == -1) and got[2]["n_rounds"] == 1
    _assert_equal(_call(e, nc.case("dropped"), max_size=8), nc.case_reference("dropped"), "max_size at the size")
    for bad in (dict(tol=-1.0), dict(tol=float("nan")), dict(eps_angle=-0.1), dict(eps_angle=float("nan"))):
        with pytest.raises(_lib.MgicpError) as err:
            _call(e, c, **bad)
        assert err.value.code == _lib.MGICP_E_INVALID
    # bad strides and pointers, through the C call itself
    lab, idx, off = np.zeros(100, np.int32), np.zeros(100, np.int32), np.zeros(101, np.uintp)
    for xs, ns_, nptr in ((8, 12, c.normals.ctypes.data), (12, 14, c.normals.ctypes.data), (12, 12, None)):
        rc_ = e._lib.mgicp_normal_clusters(e._h, c.xyz.ctypes.data, 100, xs, nptr, ns_, nc.TOL, nc.EPS, 1, 0,
                                           lab.ctypes.data, idx.ctypes.data, off.ctypes.data, None)
        assert rc_ == _lib.MGICP_E_INVALID


def test_strided_records_give_the_same_clusters():
    """records of 32 bytes and normals of 16, the floats between them NaN, through the C call itself"""
    e, c, ref = _engine(), nc.case("bridge"), nc.case_reference("bridge")
    n = len(c.xyz)
    rec = np.full((n, 8), np.nan, np.float32)
    rec[:, :3] = c.xyz
    nrm4 = np.full((n, 4), np.nan, np.float32)
    nrm4[:, :3] = c.normals
    lab, idx, off = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.uintp)
    rc_ = e._lib.mgicp_normal_clusters(e._h, rec.ctypes.data, n, 32, nrm4.ctypes.data, 16, c.tol, c.eps_angle,
                                       c.min_size, c.max_size, lab.ctypes.data, idx.ctypes.data, off.ctypes.data, None)
    assert rc_ == 0
    assert lab.tobytes() == ref.labels.tobytes() and idx[:len(ref.indices)].tobytes() == ref.indices.tobytes()
    assert off[:len(ref.offsets)].tolist() == ref.offsets.tolist()


def test_the_calls_leave_a_set_source_and_target_alone(cube_clouds):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, _T = cube_clouds
    c, ref = nc.case("line_middle"), nc.case_reference("line_middle")
    with GICPEngine() as e:
        e.set_source_xyz(src)
        e.set_target_xyz(tgt)
        before = e.align().copy()
        res_before = dict(e.last_result)
        got = e.normal_clusters(c.xyz, c.normals, c.tol, c.eps_angle, c.min_size, c.max_size)
        e.dominant_normals(c.normals, got[0])
        after = e.align()
        assert after.tobytes() == before.tobytes()
        assert e.last_result["iterations"] == res_before["iterations"]
    _assert_equal(got, ref, "beside a set source and target")


# ---- dominant normals ------------------------------------------------------------------------------------------
def test_dominant_normals_equal_the_tree_restatement():
    e = _engine()
    normals, clusters = nc.dominant_case()
    want, _sums = nc.dominant_reference(normals, clusters)
    once, _ = nc.dominant_reference(normals, clusters, first_twice=False)
    got = e.dominant_normals(normals, clusters)
    for c, size in enumerate(nc.DOMINANT_SIZES):
        assert got[c].tobytes() == want[c].tobytes(), size
        if size > 1:  # a single member's normal is itself either way
            assert got[c].tobytes() != once[c].tobytes(), size
    nrm4 = np.full((len(normals), 4), np.nan, np.float32)
    nrm4[:, :3] = normals
    assert e.dominant_normals(nrm4, clusters).tobytes() == got.tobytes()
    assert e.dominant_normals(normals, clusters).tobytes() == got.tobytes()


def test_dominant_normals_of_nan_zero_and_bad_clusters():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    normals = np.float32([[0, 0, 1], [np.nan, 0, 1], [0, 0, -1], [0, 3, 4]])
    got = e.dominant_normals(normals, [[0, 1], [0, 2, 2], [3], [2, 0]])
    assert np.all(np.isnan(got[0, :1])) and got[1].tolist() == [0, 0, 0]  # (0,0,1) twice and (0,0,-1) twice: left as it is
    assert got[2].tobytes() == np.float32([0, 0.6, 0.8]).tobytes() and got[3].tolist() == [0, 0, -1]
    assert len(e.dominant_normals(normals, [])) == 0
    for bad in ([[0], []], [[4]], [[-1, 0]]):
        with pytest.raises(_lib.MgicpError) as err:
            e.dominant_normals(normals, bad)
        assert err.value.code == _lib.MGICP_E_INVALID


def test_python_mirror_of_the_normals_method():
    """obtainNormalsCluster's parameters and fallback, obtainDominantNormals, and the chain"""
    from leica_point_cloud_processing_amd import initial_alignment as ia

    e = _engine()
    c = nc.case("patch_unit")
    assert [m.tolist() for m in ia.obtainNormalsCluster(c.xyz, c.normals, e)] == [list(range(100))]
    a = nc.case("patch_above_one")  # 100 singletons below min_size 2: the fallback of one cluster 0 .. n - 1
    clusters = ia.obtainNormalsCluster(a.xyz, a.normals, e)
    assert [m.tolist() for m in clusters] == [list(range(100))]
    dom = ia.obtainDominantNormals(a.normals, clusters, e)
    assert dom.tobytes() == nc.dominant_reference(a.normals, clusters)[0].tobytes()


def test_run_normals_based_algorithm_equals_its_members():
    from leica_point_cloud_processing_amd import initial_alignment as ia
    from leica_point_cloud_processing_amd import synth

    e = _engine()
    scan, cad, _T = synth.scan_vs_cad(3000, 3000)
    pairs = []
    for cloud in (scan, cad):  # quarter scale: the 5 cm tolerance then spans several records
        xyz = np.ascontiguousarray(cloud * np.float32(0.25), np.float32)
        pairs.append((xyz, e.estimate_normals(xyz, 10.0 * e.cloud_resolution(xyz))[0]))
    src_dom, tgt_dom, steps = ia.runNormalsBasedAlgorithm(pairs[0], pairs[1], e)
    for name, (xyz, nrm), dom in (("source", pairs[0], src_dom), ("target", pairs[1], tgt_dom)):
        _st, _kp, non = ia.obtainBoundaryKeypoints(xyz, nrm, e)
        assert steps[name + "_non_boundary_indices"].tobytes() == non.tobytes()
        clusters = ia.obtainNormalsCluster(xyz[non], nrm[non], e)
        assert [m.tobytes() for m in steps[name + "_cluster_indices"]] == [m.tobytes() for m in clusters]
        assert dom.tobytes() == ia.obtainDominantNormals(nrm[non], clusters, e).tobytes()
        assert dom.shape == (len(clusters), 3) and len(clusters) >= 1
