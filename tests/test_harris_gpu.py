"""mgicp_harris_keypoints (pcl::HarrisKeypoint3D with a radius search, InitialAlignment::obtainHarrisKeypoints)
on the GPU against the NumPy / SciPy reference of tests/harris_cases.py, in layers:

  1. n_neighbors and n_finite are exact;
  2. covar: a firm entry (harris_cases: the correctly rounded float is decided) equals float32(exact) bit for
     bit, any other entry lies within one ulp of it;
  3. response is the header's float32 expression applied to the engine's OWN covar, bit for bit (the NumPy
     float32 model: exact only if the kernel contracts nothing);
  4. keypoints is the header's rule applied to the engine's OWN response over the reference's sets, exactly and
     in order, and the counters agree.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import harris_cases as hc
from conftest import ROOT

pytestmark = pytest.mark.gpu

_ENGINE = []
_RUNS = {}


def _engine():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    if not _ENGINE:
        _ENGINE.append(GICPEngine())
    return _ENGINE[0]


def _call(e, name):
    xyz, nrm, radius, thr, nonmax = hc.case(name)
    return e.harris_keypoints(xyz, nrm, radius, thr, bool(nonmax), want_response=True, want_covar=True,
                              want_counts=True)


def _run(name):
    """the engine's outputs for a case (every output asked for), computed once and shared"""
    if name not in _RUNS:
        _RUNS[name] = _call(_engine(), name)
    return _RUNS[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same_floats(a, b, msg=""):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    ok = ~np.isnan(a)
    np.testing.assert_array_equal(_bits(a[ok]), _bits(b[ok]), err_msg=msg)


def _raw(e, xyz, nrm, radius, thr, nonmax=1, n=None, stride=None, nstride=None, src=True, nsrc=True, kp=True,
         nk=True, resp=False, cov=False, cnt=False, info=False, ctx=True):
    """the C call itself with any of the optional outputs NULL: (status, keypoints, response, covar, counts)"""
    from leica_point_cloud_processing_amd import _lib

    n = len(xyz) if n is None else n
    k = np.full(max(n, 1), -7, np.int32)
    r = np.zeros(max(n, 1), np.float32)
    c = np.zeros((max(n, 1), 6), np.float32)
    m = np.zeros(max(n, 1), np.int32)
    count = ctypes.c_size_t(12345)
    hi = _lib.MgicpHarrisInfo()
    rc = e._lib.mgicp_harris_keypoints(
        e._h if ctx else None, ctypes.c_void_p(xyz.ctypes.data) if src else None, n,
        xyz.strides[0] if stride is None else stride, ctypes.c_void_p(nrm.ctypes.data) if nsrc else None,
        nrm.strides[0] if nstride is None else nstride, float(radius), float(thr), nonmax,
        ctypes.c_void_p(k.ctypes.data) if kp else None, ctypes.byref(count) if nk else None,
        ctypes.c_void_p(r.ctypes.data) if resp else None, ctypes.c_void_p(c.ctypes.data) if cov else None,
        ctypes.c_void_p(m.ctypes.data) if cnt else None, ctypes.byref(hi) if info else None)
    return rc, k[:count.value] if rc == 0 else k[:0], r[:n], c[:n], m[:n]


@pytest.mark.parametrize("name", hc.CASES)
def test_set_sizes_are_exact(name):
    ref = hc.case_reference(name)
    _kp, _resp, _cov, cnt, info = _run(name)
    np.testing.assert_array_equal(cnt, ref.count)
    assert info["n_finite"] == ref.n_finite
    assert info["pair_tests"] >= len(ref.I)


@pytest.mark.parametrize("name", hc.CASES)
def test_covar_is_the_correctly_rounded_mean_where_that_is_decided(name):
    ref = hc.case_reference(name)
    cov = _run(name)[2]
    assert cov.shape == (ref.n, 6)
    print(f"{name}: non-firm share {hc.nonfirm_share(ref):.2e}")
    assert hc.nonfirm_share(ref) <= hc.NONFIRM_CAP
    want = ref.covar
    _same_floats(cov[ref.firm], want[ref.firm], name)
    loose = ~ref.firm
    with np.errstate(invalid="ignore"):
        near = ((cov == want) | (cov == np.nextafter(want, np.float32(np.inf))) |
                (cov == np.nextafter(want, np.float32(-np.inf))))
    assert near[loose].all(), name
    assert (cov[~ref.finite] == 0).all()


@pytest.mark.parametrize("name", hc.CASES)
def test_response_is_the_float_expression_of_the_engines_covar(name):
    ref = hc.case_reference(name)
    _kp, resp, cov, _cnt, _info = _run(name)
    _same_floats(resp, hc.response_model(cov), name)
    assert (_bits(resp[~ref.finite]) == 0).all()


@pytest.mark.parametrize("name", hc.CASES)
def test_keypoints_follow_the_rule_on_the_engines_response(name):
    _xyz, _nrm, _radius, thr, nonmax = hc.case(name)
    ref = hc.case_reference(name)
    kp, resp, _cov, _cnt, info = _run(name)
    want, cand, tied = hc.keypoint_rule(ref, resp, thr, bool(nonmax))
    assert kp.dtype == np.int32
    np.testing.assert_array_equal(kp, want)
    assert info["n_candidates"] == cand.sum() and info["n_keypoints"] == len(want) and info["n_tied"] == tied.sum()
    if name in hc.NMS_CASES:      # with the engine's response too: keypoints, and candidates that lost
        assert 0 < len(want) < cand.sum()


@pytest.mark.parametrize("name", ("part_1p4", "cube_3", "nonfinite", "clump"))
def test_repeated_and_output_free_calls_give_the_same_bits(name):
    e = _engine()
    xyz, nrm, radius, thr, nonmax = hc.case(name)
    kp, resp, cov, cnt, info = _run(name)
    kp2, resp2, cov2, cnt2, info2 = _call(e, name)
    np.testing.assert_array_equal(kp2, kp)
    np.testing.assert_array_equal(_bits(resp2), _bits(resp))
    np.testing.assert_array_equal(_bits(cov2), _bits(cov))
    np.testing.assert_array_equal(cnt2, cnt)
    for f in ("n_finite", "n_candidates", "n_keypoints", "n_tied", "pair_tests"):
        assert info2[f] == info[f], f
    rc, kp3, _r, _c, _m = _raw(e, xyz, np.ascontiguousarray(nrm), radius, thr, nonmax)
    assert rc == 0
    np.testing.assert_array_equal(kp3, kp)


@pytest.mark.parametrize("name", ("nonfinite", "flat"))
def test_nonfinite_records_do_not_disturb_the_finite_ones(name):
    xyz, nrm, radius, thr, nonmax = hc.case(name)
    fin = np.isfinite(xyz).all(1)
    kp, resp, cov, cnt, _info = _run(name)
    assert fin[kp].all() and (cnt[~fin] == 0).all()
    kp2, resp2, cov2, cnt2, info2 = _engine().harris_keypoints(xyz[fin], nrm[fin], radius, thr, bool(nonmax),
                                                               want_response=True, want_covar=True, want_counts=True)
    np.testing.assert_array_equal(np.flatnonzero(fin)[kp2], kp)
    np.testing.assert_array_equal(_bits(resp2), _bits(resp[fin]))
    np.testing.assert_array_equal(_bits(cov2), _bits(cov[fin]))
    np.testing.assert_array_equal(cnt2, cnt[fin])
    # no finite record at all
    kp, resp, cov, cnt, info = _engine().harris_keypoints(np.full((5, 3), np.nan, np.float32), np.ones((5, 3), np.float32),
                                                          0.1, -1.0, True, want_response=True, want_covar=True,
                                                          want_counts=True)
    assert len(kp) == 0 and (resp == 0).all() and (cov == 0).all() and (cnt == 0).all()
    assert info["n_finite"] == 0 and info["n_candidates"] == 0 and info["n_keypoints"] == 0


def test_threshold_at_a_response_and_one_step_above():
    """the threshold test is !(response < threshold): a record whose response equals the threshold stays, one
    float step above it is gone"""
    e = _engine()
    xyz, nrm, radius, _thr, _nm = hc.case("part_3")
    ref = hc.case_reference("part_3")
    kp, resp, _cov, _cnt, _info = _run("part_3")
    i = int(kp[np.argmin(resp[kp])])          # the keypoint with the lowest response
    for thr, kept in ((resp[i], True), (np.nextafter(resp[i], np.float32(np.inf)), False)):
        got, r2, _c, _m, info = e.harris_keypoints(xyz, nrm, radius, thr, True, want_response=True)
        np.testing.assert_array_equal(_bits(r2), _bits(resp))
        want, cand, tied = hc.keypoint_rule(ref, resp, thr)
        np.testing.assert_array_equal(got, want)
        assert (i in got.tolist()) == kept
        assert info["n_candidates"] == cand.sum() and info["n_tied"] == tied.sum()


def test_pcl_records_with_poisoned_padding():
    """32-byte pcl::PointXYZRGB and pcl::Normal records, NaN in every byte the call must step over"""
    e = _engine()
    xyz, nrm, radius, thr, _nm = hc.case("part_1p4")
    kp, resp, cov, cnt, _info = _run("part_1p4")
    prec = np.full((len(xyz), 8), np.nan, np.float32)
    prec[:, :3] = xyz
    nrec = np.full((len(xyz), 8), np.nan, np.float32)
    nrec[:, :3] = nrm
    rc, k2, r2, c2, m2 = _raw(e, prec, nrec, radius, thr, resp=True, cov=True, cnt=True)
    assert rc == 0 and prec.strides[0] == 32 and nrec.strides[0] == 32
    np.testing.assert_array_equal(k2, kp)
    np.testing.assert_array_equal(_bits(r2), _bits(resp))
    np.testing.assert_array_equal(_bits(c2), _bits(cov))
    np.testing.assert_array_equal(m2, cnt)
    four = np.concatenate([nrm, np.full((len(xyz), 1), np.nan, np.float32)], 1)      # getNormals' [n, 4]
    k3 = e.harris_keypoints(xyz, four, radius, thr)[0]
    np.testing.assert_array_equal(k3, kp)


def test_list_entries_after_the_count_and_nonmax_off():
    e = _engine()
    xyz, nrm, radius, thr, _nm = hc.case("part_1p4")
    kp = _run("part_1p4")[0]
    from leica_point_cloud_processing_amd import _lib

    buf = np.full(len(xyz), -7, np.int32)
    count = ctypes.c_size_t()
    rc = e._lib.mgicp_harris_keypoints(e._h, ctypes.c_void_p(xyz.ctypes.data), len(xyz), 12,
                                       ctypes.c_void_p(nrm.ctypes.data), 12, float(radius), float(thr), 1,
                                       ctypes.c_void_p(buf.ctypes.data), ctypes.byref(count), None, None, None, None)
    assert rc == _lib.MGICP_OK and count.value == len(kp)
    np.testing.assert_array_equal(buf[:len(kp)], kp)
    assert (buf[len(kp):] == -1).all()
    # nonmax = 0: every record, the first sweep's outputs unchanged
    allkp, resp, _c, _m, info = _run("part_all")
    np.testing.assert_array_equal(allkp, np.arange(len(xyz)))
    np.testing.assert_array_equal(_bits(resp), _bits(_run("part_1p4")[1]))
    assert info["n_tied"] == 0 and info["n_candidates"] == _run("part_1p4")[4]["n_candidates"]
    assert info["pair_tests"] < _run("part_1p4")[4]["pair_tests"]


def test_set_source_and_target_survive(cube_clouds):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, _ = cube_clouds
    e = GICPEngine()
    e.set_source_xyz(src)
    e.set_target_xyz(tgt)
    T0 = e.align()
    for name in ("part_1p4", "clump"):
        kp, resp, cov, _cnt, _info = _call(e, name)
        np.testing.assert_array_equal(kp, _run(name)[0])
        np.testing.assert_array_equal(_bits(resp), _bits(_run(name)[1]))
        np.testing.assert_array_equal(_bits(cov), _bits(_run(name)[2]))
    T1 = e.align()
    np.testing.assert_array_equal(_bits(T0), _bits(T1))
    e.close()


def test_invalid_arguments():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    xyz, nrm, radius, thr, _nm = hc.case("flat")
    for bad_radius in (-0.1, float("nan")):
        with pytest.raises(_lib.MgicpError) as ei:
            e.harris_keypoints(xyz, nrm, bad_radius, thr)
        assert ei.value.code == _lib.MGICP_E_INVALID
    with pytest.raises(_lib.MgicpError) as ei:
        e.harris_keypoints(xyz, nrm, radius, float("nan"))
    assert ei.value.code == _lib.MGICP_E_INVALID
    with pytest.raises(ValueError):
        e.harris_keypoints(xyz, nrm[:-1], radius, thr)
    ok, bad = _lib.MGICP_OK, _lib.MGICP_E_INVALID
    assert _raw(e, xyz, nrm, radius, thr)[0] == ok
    assert _raw(e, xyz, nrm, radius, thr, stride=8)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, stride=14)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, nstride=8)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, nstride=14)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, src=False)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, nsrc=False)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, kp=False)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, nk=False)[0] == bad
    assert _raw(e, xyz, nrm, radius, thr, ctx=False)[0] == bad
    # infinite thresholds are values, not errors: everything finite passes -inf, nothing passes +inf
    assert len(_raw(e, xyz, nrm, radius, float("-inf"))[1]) == np.isfinite(xyz).all(1).sum()
    assert len(_raw(e, xyz, nrm, radius, float("inf"))[1]) == 0
    # n = 0 is fine, with or without pointers
    rc, kp, _r, _c, _m = _raw(e, xyz, nrm, radius, thr, n=0)
    assert rc == ok and len(kp) == 0
    assert _raw(e, xyz, nrm, radius, thr, n=0, src=False, nsrc=False, kp=False)[0] == ok


def test_radius_zero_links_nothing():
    xyz, nrm, _radius, _thr, _nm = hc.case("radius_zero")
    kp, resp, cov, cnt, info = _run("radius_zero")
    assert len(kp) == 0 and (_bits(resp) == 0).all() and (_bits(cov) == 0).all() and (cnt == 0).all()
    assert info["n_candidates"] == 0
    kp, _r, _c, _m, info = _engine().harris_keypoints(xyz, nrm, 0.0, 0.0)       # a zero response is not below 0
    np.testing.assert_array_equal(kp, np.arange(len(xyz)))
    assert info["n_candidates"] == len(xyz) and info["n_tied"] == 0


def _numpy_obtainHarrisKeypoints(e, xyz, nrm, radius_factor=1.4):
    """InitialAlignment::obtainHarrisKeypoints restated over the engine's product calls"""
    if len(nrm) != len(xyz):
        return -1, np.zeros(0, np.int32)
    radius = np.float32(e.cloud_resolution(xyz) * radius_factor)
    kp = e.harris_keypoints(xyz, nrm, float(radius), np.float32(1e-6), True)[0]
    return (0 if len(kp) else -1), kp


def test_obtainHarrisKeypoints_mirror():
    from leica_point_cloud_processing_amd.cloud import PointCloudRGB
    from leica_point_cloud_processing_amd.initial_alignment import obtainHarrisKeypoints

    e = _engine()
    for name, factor in (("part_1p4", 1.4), ("cube_3", 3.0), ("nonfinite", 1.4)):
        xyz, nrm, _radius, _thr, _nm = hc.case(name)
        want_status, want = _numpy_obtainHarrisKeypoints(e, xyz, nrm, factor)
        status, kp = obtainHarrisKeypoints(PointCloudRGB.from_xyz(xyz), nrm, factor, engine=e)
        assert status == want_status == 0 and kp.dtype == np.int32 and len(kp) > 0
        np.testing.assert_array_equal(kp, want)
        # the rule itself, at the mirror's float radius
        radius = float(np.float32(e.cloud_resolution(xyz) * factor))
        ref = hc.reference(xyz, nrm, radius)
        resp = e.harris_keypoints(xyz, nrm, radius, hc.THRESHOLD, want_response=True)[1]
        np.testing.assert_array_equal(kp, hc.keypoint_rule(ref, resp, hc.THRESHOLD)[0])
    xyz, nrm, _radius, _thr, _nm = hc.case("part_1p4")
    status, kp2 = obtainHarrisKeypoints(xyz, np.concatenate([nrm, nrm[:, :1]], 1), engine=e)
    assert status == 0
    np.testing.assert_array_equal(kp2, _numpy_obtainHarrisKeypoints(e, xyz, nrm)[1])
    # -1: normals that do not match the cloud; no keypoint found (no normal at all, or an empty cloud)
    status, kp = obtainHarrisKeypoints(xyz, nrm[:-1], engine=e)
    assert status == -1 and len(kp) == 0
    status, kp = obtainHarrisKeypoints(xyz, np.full_like(nrm, np.nan), engine=e)
    assert status == -1 and len(kp) == 0
    status, kp = obtainHarrisKeypoints(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), engine=e)
    assert status == -1 and len(kp) == 0


def test_adapter_obtainHarrisKeypoints_replay(tmp_path):
    """adapter/InitialAlignment_mi355x.cpp through its C++ driver: the index list of the Python mirror,
    and the keypoint cloud Filter::extractIndices makes of it."""
    from leica_point_cloud_processing_amd.initial_alignment import obtainHarrisKeypoints

    exe = os.path.join(ROOT, "adapter", "build", "replay_test_harris")
    assert os.path.exists(exe), "build it with `make harris-replay`"
    for name, factor in (("part_1p4", 1.4), ("nonfinite", 3.0)):
        xyz, nrm, _radius, _thr, _nm = hc.case(name)
        files = [tmp_path / f for f in ("cloud.bin", "normals.bin", "kp.bin")]
        np.ascontiguousarray(xyz, np.float32).tofile(files[0])
        np.ascontiguousarray(nrm, np.float32).tofile(files[1])
        r = subprocess.run([exe, str(files[0]), str(files[1]), repr(factor), str(files[2])], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr[-4000:]
        checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines())
                  if len(p) == 2 and p[1] in ("ok", "FAIL")}
        assert len(checks) >= 5 and all(checks.values()), checks
        status, kp = obtainHarrisKeypoints(xyz, nrm, factor, engine=_engine())
        assert status == 0
        np.testing.assert_array_equal(np.fromfile(files[2], np.int32), kp)
        assert f"keypoints {len(kp)} status 0" in r.stdout
