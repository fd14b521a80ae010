"""mgicp_estimate_normals (pcl::NormalEstimation with a radius search, Utils::getNormals) on the GPU
against the NumPy / SciPy reference of tests/normals_cases.py.

Exact where the quantity is exact: neighbour counts, the NaN mask, the call's counters, the bits of a
repeated call.  Directions are held to 2^-22 / gap_rel of the fp64 normal of the same neighbour set --
the bound of the specified arithmetic (a few fp64 roundings per term of C, the eigenvector moving by at
most |dC| / gap, float rounding of the output) -- and, per case, to the MEDIAN error of PCL's own float
arithmetic on the same records: where the engine deviates from PCL it does so towards the truth.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import normals_cases as nc
from conftest import ROOT

pytestmark = pytest.mark.gpu

_ENGINE = []
_RUNS = {}


def _engine():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    if not _ENGINE:
        _ENGINE.append(GICPEngine())
    return _ENGINE[0]


def _run(name):
    """the engine's outputs for a direction case, computed once and shared"""
    if name not in _RUNS:
        xyz, radius = nc.case(name)
        _RUNS[name] = _engine().estimate_normals(xyz, radius)
    return _RUNS[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same_bits(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(_bits(x), _bits(y))


def _nan_rows(normals):
    return np.isnan(normals).any(1)


@pytest.mark.parametrize("name", nc.DIRECTION_CASES)
def test_counts_mask_and_counters_are_exact(name):
    xyz, radius = nc.case(name)
    ref = nc.case_reference(name)
    normals, curvature, count, info = _run(name)
    assert normals.shape == (len(xyz), 3) and normals.dtype == np.float32
    assert curvature.shape == (len(xyz),) and curvature.dtype == np.float32 and count.dtype == np.int32
    np.testing.assert_array_equal(count, ref.count)
    nan = _nan_rows(normals)
    np.testing.assert_array_equal(nan, ~ref.has)
    assert np.isnan(normals[nan]).all()          # all three components
    np.testing.assert_array_equal(np.isnan(curvature), nan)
    np.testing.assert_array_equal(nan, ~_engine().radius_filter(xyz, radius, 3))
    assert info["n_nan"] == (~ref.has).sum()
    assert info["n_finite"] == np.isfinite(xyz).all(1).sum()
    assert info["pair_tests"] >= ref.count.sum()  # every neighbour pair was tested at least once
    assert info["ms_total"] >= info["ms_device"] >= 0 and info["ms_grid"] >= 0
    # every finite normal is a unit vector up to the float rounding of its three components
    norm = np.linalg.norm(normals[~nan].astype(np.float64), axis=1)
    print(name, "norm error", float(np.abs(norm - 1).max()), "pair tests", info["pair_tests"], "neighbour pairs",
          int(ref.count.sum()), "ms_device", info["ms_device"])
    assert np.abs(norm - 1).max() <= nc.NORM_BOUND
    # a second call gives the same bits in every output
    _same_bits(_engine().estimate_normals(xyz, radius), (normals, curvature, count))


@pytest.mark.parametrize("name", nc.DIRECTION_CASES)
def test_direction(name):
    ref = nc.case_reference(name)
    normals, _curvature, _count, _info = _run(name)
    sel = ref.has & (ref.gap_rel >= nc.GAP_MIN)
    ang = nc._angle(normals[sel].astype(np.float64), ref.normal[sel])
    pcl_median = float(np.median(ref.pcl_angle[sel]))
    print(name, "compared", int(sel.sum()), "of", int(ref.has.sum()), "worst angle", float(ang.max()),
          "worst angle * gap", float((ang * ref.gap_rel[sel]).max()), "pcl median", pcl_median)
    assert (ang <= nc.DIR_BOUND / ref.gap_rel[sel]).all()
    assert ang.max() <= pcl_median


@pytest.mark.parametrize(
    "name,viewpoint", [(n, None) for n in nc.DIRECTION_CASES] + list(nc.viewpoints().items()),
    # `part` keeps the id it had when it was the only case with a viewpoint of its own (the 8th parameter set)
    ids=[f"{n}-None" for n in nc.DIRECTION_CASES] + ["part-viewpoint7" if n == "part" else f"{n}-viewpoint" for n in nc.viewpoints()])
def test_sign(name, viewpoint):
    xyz, radius = nc.case(name)
    ref = nc.case_reference(name)
    if viewpoint is None:
        normals = _run(name)[0]
        vp = (0.0, 0.0, 0.0)
    else:
        normals = _engine().estimate_normals(xyz, radius, viewpoint)[0]
        vp = viewpoint
        # the viewpoint only flips: same components up to the sign as with the default one
        np.testing.assert_array_equal(_bits(np.abs(normals)), _bits(np.abs(_run(name)[0])))
        assert (np.signbit(normals) != np.signbit(_run(name)[0])).any()
    has = ref.has
    assert (nc.view_dot(xyz, normals, vp)[has] >= 0).all()
    sign, cos = nc.orientation(xyz, ref, vp)
    sel = has & (cos >= nc.COS_MIN)
    oriented = ref.normal * sign[:, None]
    assert ((normals[sel].astype(np.float64) * oriented[sel]).sum(1) > 0).all()


@pytest.mark.parametrize("name", nc.DIRECTION_CASES)
def test_curvature(name):
    ref = nc.case_reference(name)
    curvature = _run(name)[1]
    err = np.abs(curvature[ref.has].astype(np.float64) - ref.curvature[ref.has])
    print(name, "worst curvature error", float(err.max()))
    assert err.max() <= nc.CURV_BOUND
    assert (curvature[ref.has] >= 0).all()


def test_nonfinite_records_do_not_disturb_the_finite_ones():
    xyz, radius = nc.case("nonfinite")
    fin = np.isfinite(xyz).all(1)
    normals, curvature, count, _ = _run("nonfinite")
    assert np.isnan(normals[~fin]).all() and np.isnan(curvature[~fin]).all() and (count[~fin] == 0).all()
    alone = _engine().estimate_normals(xyz[fin], radius)
    _same_bits((normals[fin], curvature[fin], count[fin]), alone)
    n_all, c_all, k_all, info = _engine().estimate_normals(np.full((5, 3), np.nan, np.float32), radius)
    assert np.isnan(n_all).all() and np.isnan(c_all).all() and (k_all == 0).all()
    assert info["n_finite"] == 0 and info["n_nan"] == 5


def test_edge_values():
    e = _engine()
    for name, (xyz, radius) in nc.edge_clouds().items():
        ref = nc.reference(xyz, radius)
        normals, curvature, count, info = e.estimate_normals(xyz, radius)
        assert normals.shape == (len(xyz), 3) and len(curvature) == len(count) == len(xyz), name
        np.testing.assert_array_equal(count, ref.count, err_msg=name)
        if name == "denormal_r2":  # three identical points have no plane: NaN or some unit vector
            np.testing.assert_array_equal(_nan_rows(normals)[~ref.has], True)
            fin = ~_nan_rows(normals)
            assert (np.abs(np.linalg.norm(normals[fin].astype(np.float64), axis=1) - 1) <= 1e-6).all()
        else:
            assert np.isnan(normals).all() and np.isnan(curvature).all(), name
            assert info["n_nan"] == len(xyz), name
        assert info["n_finite"] == len(xyz), name
    assert (e.estimate_normals(*nc.edge_clouds()["radius_zero"])[2] == 0).all()


def test_invalid_arguments():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    xyz, _ = nc.case("huge_radius")
    for radius in (-1.0, float("nan")):
        with pytest.raises(_lib.MgicpError) as ei:
            e.estimate_normals(xyz, radius)
        assert ei.value.code == _lib.MGICP_E_INVALID
    out = np.zeros((len(xyz), 3), np.float32)
    call = e._lib.mgicp_estimate_normals
    args = lambda stride, nstride, src=xyz.ctypes.data, dst=out.ctypes.data: (  # noqa: E731
        e._h, ctypes.c_void_p(src), len(xyz), stride, 1.0, None, ctypes.c_void_p(dst), nstride, None, None, None)
    assert call(*args(12, 12)) == _lib.MGICP_OK  # curvature, n_neighbors, info and viewpoint may be NULL
    assert call(*args(8, 12)) == _lib.MGICP_E_INVALID
    assert call(*args(12, 8)) == _lib.MGICP_E_INVALID
    assert call(*args(12, 14)) == _lib.MGICP_E_INVALID
    assert call(*args(12, 12, src=None)) == _lib.MGICP_E_INVALID
    assert call(*args(12, 12, dst=None)) == _lib.MGICP_E_INVALID
    assert call(None, *args(12, 12)[1:]) == _lib.MGICP_E_INVALID


def test_null_viewpoint_is_the_origin_and_strided_records_keep_their_other_bytes():
    e = _engine()
    xyz, radius = nc.case("huge_radius")
    _same_bits(e.estimate_normals(xyz, radius, (0.0, 0.0, 0.0)), _run("huge_radius"))
    # pcl::Normal's 32-byte records: x, y, z written, every other byte left as it was
    rec = np.full((len(xyz), 8), 7.0, np.float32)
    rc = e._lib.mgicp_estimate_normals(e._h, ctypes.c_void_p(xyz.ctypes.data), len(xyz), 12, float(radius), None,
                                       ctypes.c_void_p(rec.ctypes.data), 32, None, None, None)
    assert rc == 0
    np.testing.assert_array_equal(_bits(rec[:, :3]), _bits(_run("huge_radius")[0]))
    assert (rec[:, 3:] == 7.0).all()


def test_set_source_and_target_survive(cube_clouds):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, _ = cube_clouds
    e = GICPEngine()
    e.set_source_xyz(src)
    e.set_target_xyz(tgt)
    T0 = e.align()
    xyz, radius = nc.case("huge_radius")
    _same_bits(e.estimate_normals(xyz, radius), _run("huge_radius"))
    T1 = e.align()
    np.testing.assert_array_equal(_bits(T0), _bits(T1))
    e.close()


def test_degenerate_sets_return():
    xyz, radius, rows = nc.degenerate()
    normals, curvature, count, _ = _engine().estimate_normals(xyz, radius)
    np.testing.assert_array_equal(count, nc.reference(xyz, radius).count)
    n = normals[rows].astype(np.float64)
    nan = np.isnan(n).any(1)
    assert (np.abs(np.linalg.norm(n[~nan], axis=1) - 1) <= 1e-6).all()
    assert len(curvature) == len(xyz)


def test_getNormals_mirror():
    from leica_point_cloud_processing_amd.cloud import PointCloudRGB
    from leica_point_cloud_processing_amd.gicp_alignment import getNormals

    xyz, radius = nc.case("part_small")
    normals, curvature, _count, _ = _run("part_small")
    ok, out = getNormals(PointCloudRGB.from_xyz(xyz), radius, engine=_engine())
    assert ok and out.shape == (len(xyz), 4) and out.dtype == np.float32
    np.testing.assert_array_equal(_bits(out[:, :3]), _bits(normals))
    np.testing.assert_array_equal(_bits(out[:, 3]), _bits(curvature))
    ok, out = getNormals(np.zeros((0, 3), np.float32), radius, engine=_engine())
    assert ok and out.shape == (0, 4)


def test_adapter_getNormals_replay(tmp_path):
    """adapter/Utils_mi355x.cpp through its C++ driver: pcl::Normal records bit for bit those of
    GICPEngine.estimate_normals, is_dense against the NaN mask."""
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_normals")
    assert os.path.exists(exe), "build it with `make normals-replay`"
    xyz, radius = nc.case("part_small")
    src, dst = tmp_path / "cloud.bin", tmp_path / "normals.bin"
    np.ascontiguousarray(xyz, np.float32).tofile(src)
    r = subprocess.run([exe, str(src), str(dst), repr(float(radius))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines()) if len(p) == 2 and p[1] in ("ok", "FAIL")}
    assert checks and all(checks.values()), checks
    rec = np.fromfile(dst, np.float32).reshape(-1, 8)
    normals, curvature, _count, _ = _run("part_small")
    assert len(rec) == len(xyz)
    np.testing.assert_array_equal(_bits(rec[:, :3]), _bits(normals))
    np.testing.assert_array_equal(_bits(rec[:, 4]), _bits(curvature))
    assert (rec[:, 3] == 0).all() and (rec[:, 5:] == 0).all()
    nan = _nan_rows(normals)
    assert nan.any()
    assert f"normals {len(xyz)} width {len(xyz)} height 1 dense 0" in r.stdout
    # a dense result, at the radius InitialAlignment's constructor derives from the cloud's resolution
    cube, _ = nc.case("cube")
    np.ascontiguousarray(cube, np.float32).tofile(src)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert f"normals {len(cube)} width {len(cube)} height 1 dense 1" in r.stdout
    radius = float([line.split()[1] for line in r.stdout.splitlines() if line.startswith("radius ")][0])
    rec = np.fromfile(dst, np.float32).reshape(-1, 8)
    n2, c2, _k, _ = _engine().estimate_normals(cube, radius)
    np.testing.assert_array_equal(_bits(rec[:, :3]), _bits(n2))
    np.testing.assert_array_equal(_bits(rec[:, 4]), _bits(c2))
