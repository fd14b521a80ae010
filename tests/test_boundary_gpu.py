"""mgicp_boundary_points (pcl::BoundaryEstimation with a k-search, InitialAlignment::obtainBoundaryKeypoints)
on the GPU against the NumPy / SciPy reference of tests/boundary_cases.py.

Exact where the quantity is exact: the neighbour sets in (d2, original index) order, the records that are
never boundary points, boundary == (max_gap > float(threshold)), the call's counters, the bits of a repeated
call and of the calls that leave outputs out (those run the logged kernel and its hand-off instead of the
sorted-list kernel: the same sets by another route).  The gap itself is held to
BOUND_i = 2^-20 (1 + sens_i) of the fp64 truth of the same set, the flags to the truth's wherever the truth
is farther than that from the threshold.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import boundary_cases as bc
import normals_cases as nc
from conftest import ROOT

pytestmark = pytest.mark.gpu

_ENGINE = []
_RUNS = {}
THR_F = np.float32(bc.THRESHOLD)


def _engine():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    if not _ENGINE:
        _ENGINE.append(GICPEngine())
    return _ENGINE[0]


def _run(name):
    """the engine's outputs for a case (every output asked for), computed once and shared"""
    if name not in _RUNS:
        xyz, nrm, k = bc.case(name)
        _RUNS[name] = _engine().boundary_points(xyz, nrm, k, bc.THRESHOLD, want_gap=True, want_indices=True)
    return _RUNS[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == bool else a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _raw(e, xyz, nrm, k, thr, gap=False, nn=False, info=False, nstride=None, stride=12, n=None, src=True, nsrc=True,
         flags=True, ctx=True):
    """the C call itself with any of the optional outputs NULL: (status, flags, gap, nn)"""
    from leica_point_cloud_processing_amd import _lib

    n = len(xyz) if n is None else n
    nrm = np.ascontiguousarray(nrm, np.float32)
    f = np.zeros(max(n, 1), np.uint8)
    g = np.zeros(max(n, 1), np.float32)
    ix = np.zeros((max(n, 1), max(k, 1)), np.int32)
    bi = _lib.MgicpBoundaryInfo()
    rc = e._lib.mgicp_boundary_points(
        e._h if ctx else None, ctypes.c_void_p(xyz.ctypes.data) if src else None, n, stride,
        ctypes.c_void_p(nrm.ctypes.data) if nsrc else None, nrm.strides[0] if nstride is None else nstride, k, thr,
        ctypes.c_void_p(f.ctypes.data) if flags else None, ctypes.c_void_p(g.ctypes.data) if gap else None,
        ctypes.c_void_p(ix.ctypes.data) if nn else None, ctypes.byref(bi) if info else None)
    return rc, f[:n].astype(bool), g[:n], ix[:n]


@pytest.mark.parametrize("name", bc.CASES)
def test_sets_rules_flags_and_counters_are_exact(name):
    xyz, nrm, k = bc.case(name)
    ref = bc.case_reference(name)
    n = len(xyz)
    e = _engine()
    flags, gap, nn, info = _run(name)
    assert flags.shape == (n,) and flags.dtype == bool
    assert gap.shape == (n,) and gap.dtype == np.float32 and nn.shape == (n, k) and nn.dtype == np.int32
    # the sets, in (d2, original index) order, -1 padded; all -1 for a non-finite record
    np.testing.assert_array_equal(nn, ref.nn)
    # never a boundary point: exactly the four rules
    np.testing.assert_array_equal(np.isnan(gap), ~ref.decided)
    assert not flags[~ref.decided].any()
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(flags, gap > THR_F)
    assert (gap[ref.decided] >= bc.FLT_MIN).all()
    fin = np.isfinite(xyz).all(1)
    assert info["n_finite"] == fin.sum()
    assert info["n_boundary"] == flags.sum()
    assert info["n_undecided"] == (fin & ~ref.decided).sum()
    assert info["pair_tests"] >= ref.size.sum()  # every member was tested at least once
    assert info["ms_total"] >= info["ms_device"] >= 0 and info["ms_grid"] >= 0
    print(name, "boundary", int(flags.sum()), "undecided", int(info["n_undecided"]), "pair tests", info["pair_tests"],
          "members", int(ref.size.sum()), "ms_device", info["ms_device"])
    # a second call gives the same bits in every output
    f2, g2, nn2, info2 = e.boundary_points(xyz, nrm, k, bc.THRESHOLD, want_gap=True, want_indices=True)
    np.testing.assert_array_equal(f2, flags)
    np.testing.assert_array_equal(_bits(g2), _bits(gap))
    np.testing.assert_array_equal(nn2, nn)
    assert info2["pair_tests"] == info["pair_tests"]
    # without the indices (the logged kernel and its hand-off): the same flags and the same gap bits, twice
    for _ in range(2):
        f3, g3, nn3, info3 = e.boundary_points(xyz, nrm, k, bc.THRESHOLD, want_gap=True)
        assert nn3 is None
        np.testing.assert_array_equal(f3, flags)
        np.testing.assert_array_equal(_bits(g3), _bits(gap))
        assert info3["n_boundary"] == info["n_boundary"] and info3["n_undecided"] == info["n_undecided"]
        assert info3["pair_tests"] >= ref.size[ref.decided].sum()
    # max_gap, nn_indices and info NULL, one at a time and all together
    for kw in ({"gap": True, "nn": True}, {"nn": True, "info": True}, {"gap": True, "info": True}, {}):
        rc, f4, g4, nn4 = _raw(e, xyz, nrm, k, bc.THRESHOLD, **kw)
        assert rc == 0
        np.testing.assert_array_equal(f4, flags, err_msg=str(kw))
        if kw.get("gap"):
            np.testing.assert_array_equal(_bits(g4), _bits(gap))
        if kw.get("nn"):
            np.testing.assert_array_equal(nn4, nn)


@pytest.mark.parametrize("name", bc.CASES)
def test_gap_and_flags_within_bound_of_the_truth(name):
    ref = bc.case_reference(name)
    flags, gap, _nn, _info = _run(name)
    gap_ok, flag_ok = bc.comparable(ref)
    err = np.abs(gap.astype(np.float64) - ref.truth)
    rel = err[gap_ok] / bc.bound(ref.sens[gap_ok])
    print(name, "compared", int(gap_ok.sum()), "worst error", float(err[gap_ok].max()), "worst error / bound",
          float(rel.max()), "left out of the gaps", int((ref.decided & ~gap_ok).sum()), "of the flags",
          int((ref.decided & ~flag_ok).sum()))
    assert (err[gap_ok] <= bc.bound(ref.sens[gap_ok])).all()
    np.testing.assert_array_equal(flags[flag_ok], (ref.truth > np.float64(THR_F))[flag_ok])


@pytest.mark.parametrize("name", tuple(nc.FAR_SHEET_X0))
def test_far_sheet_by_both_routes(name):
    """far_sheet with and without nn_indices: boundary_sorted_kernel and boundary_kernel, each with the
    hand-off to boundary_wave_kernel for the queries that reach the ring cap.  At |X0| = 4096.5 the grid's slop
    exceeds every k-th neighbour distance (test_far_frame_certificates), so ordinary queries of the dense sheet
    may reach the cap while their neighbours are near; what share does cannot be certified from the CPU side
    -- the boundary grid's cell edge is auto-sized and the call has no hand-off counter -- so nothing here
    depends on it: the sets equal the reference's whichever path a query takes, and the call without the
    indices gives the same gap bits (the gap depends on the set alone) within the bound of the truth.
    Printed, not asserted: the pair_tests of the three calls and the boundary ms_device, for DESIGN.md's
    account of what the slop costs a fine cloud in a far frame (the control is the same cloud at X0 = 0)."""
    import fpfh_cases as fc

    e = _engine()
    xyz, nrm, k = bc.case(name)
    ref = bc.case_reference(name)
    gap_ok, flag_ok = bc.comparable(ref)
    runs = {}
    for want in (True, False):
        flags, gap, nn, info = e.boundary_points(xyz, nrm, k, bc.THRESHOLD, want_gap=True, want_indices=want)
        runs[want] = (flags, gap, info)
        if want:
            np.testing.assert_array_equal(nn, ref.nn)
        else:
            assert nn is None
        np.testing.assert_array_equal(np.isnan(gap), ~ref.decided)
        err = np.abs(gap.astype(np.float64) - ref.truth)
        assert (err[gap_ok] <= bc.bound(ref.sens[gap_ok])).all()
        np.testing.assert_array_equal(flags[flag_ok], (ref.truth > np.float64(THR_F))[flag_ok])
        assert info["n_finite"] == len(xyz) and info["n_undecided"] == 0 and info["pair_tests"] >= ref.size.sum()
    np.testing.assert_array_equal(_bits(runs[False][1]), _bits(runs[True][1]))
    np.testing.assert_array_equal(runs[False][0], runs[True][0])
    np.testing.assert_array_equal(_bits(runs[True][1]), _bits(_run(name)[1]))
    ninfo = e.estimate_normals(*nc.case(name))[3]
    finfo = e.fpfh_features(*fc.case(name))[3]
    print(name, "pair_tests: normals", ninfo["pair_tests"], "boundary with indices", runs[True][2]["pair_tests"],
          "without", runs[False][2]["pair_tests"], "fpfh", finfo["pair_tests"], "| ms_device: boundary with indices",
          runs[True][2]["ms_device"], "without", runs[False][2]["ms_device"], "normals", ninfo["ms_device"], "fpfh",
          finfo["ms_device"])


def test_other_thresholds():
    xyz, nrm, k = bc.case("part")
    ref = bc.case_reference("part")
    e = _engine()
    _flags, gap, _nn, _info = _run("part")
    half_pi = np.pi / 2
    f, g, _n, info = e.boundary_points(xyz, nrm, k, half_pi, want_gap=True)
    np.testing.assert_array_equal(_bits(g), _bits(gap))  # the threshold only decides
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(f, gap > np.float32(half_pi))
    _gap_ok, flag_ok = bc.comparable(ref, half_pi)
    np.testing.assert_array_equal(f[flag_ok], (ref.truth > np.float64(np.float32(half_pi)))[flag_ok])
    assert 0 < f.sum() < _run("part")[0].sum()
    for thr in (0.0, -1.0, float("-inf")):  # every decided record is a boundary point
        f, _g, _n, info = e.boundary_points(xyz, nrm, k, thr)
        np.testing.assert_array_equal(f, ref.decided)
        assert info["n_boundary"] == ref.decided.sum()
    f, _g, _n, _i = e.boundary_points(xyz, nrm, k, float("inf"))
    assert not f.any()


def test_nonfinite_records_do_not_disturb_the_finite_ones():
    xyz, nrm, k = bc.case("nonfinite")
    fin = np.isfinite(xyz).all(1)
    flags, gap, nn, _ = _run("nonfinite")
    assert not flags[~fin].any() and np.isnan(gap[~fin]).all() and (nn[~fin] == -1).all()
    f, g, ix, info = _engine().boundary_points(xyz[fin], nrm[fin], k, bc.THRESHOLD, want_gap=True, want_indices=True)
    np.testing.assert_array_equal(f, flags[fin])
    np.testing.assert_array_equal(_bits(g), _bits(gap[fin]))
    back = np.flatnonzero(fin)
    np.testing.assert_array_equal(np.where(ix >= 0, back[np.maximum(ix, 0)], -1), nn[fin])
    # the same through the logged kernel
    f2, g2, _n, _i = _engine().boundary_points(xyz[fin], nrm[fin], k, bc.THRESHOLD, want_gap=True)
    np.testing.assert_array_equal(_bits(g2), _bits(gap[fin]))
    # no finite record at all
    f, g, ix, info = _engine().boundary_points(np.full((5, 3), np.nan, np.float32), np.ones((5, 3), np.float32), 30,
                                               bc.THRESHOLD, want_gap=True, want_indices=True)
    assert not f.any() and np.isnan(g).all() and (ix == -1).all()
    assert info["n_finite"] == 0 and info["n_undecided"] == 0 and info["n_boundary"] == 0


def test_small_sizes():
    e = _engine()
    rng = np.random.default_rng(21)
    pts = np.concatenate([rng.uniform(0, 1, (3, 2)), np.zeros((3, 1))], 1).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (3, 1))
    for n in (0, 1, 2, 3):
        for k in (1, 2, 3, 30, 32):
            ref = bc.reference(pts[:n], nrm[:n], k)
            for want in (True, False):
                f, g, ix, info = e.boundary_points(pts[:n], nrm[:n], k, bc.THRESHOLD, want_gap=True, want_indices=want)
                assert f.shape == (n,) and g.shape == (n,)
                np.testing.assert_array_equal(np.isnan(g), ~ref.decided, err_msg=f"n {n} k {k}")
                if want:
                    assert ix.shape == (n, k)
                    np.testing.assert_array_equal(ix, ref.nn)
                err = np.abs(g.astype(np.float64) - ref.truth)[ref.decided]
                assert (err <= bc.bound(ref.sens[ref.decided])).all()
                assert info["n_finite"] == n and info["n_undecided"] == (~ref.decided).sum()
            # three records are a set of three only from k = 3 on; k < 3 flags nothing
            assert ref.decided.all() == (n == 3 and k >= 3) or n == 0
            if k < 3:
                assert not f.any()


def test_invalid_arguments():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    xyz, nrm, k = bc.case("huge_radius")
    for bad_k in (0, 33, -1):
        with pytest.raises(_lib.MgicpError) as ei:
            e.boundary_points(xyz, nrm, bad_k)
        assert ei.value.code == _lib.MGICP_E_INVALID
    with pytest.raises(_lib.MgicpError) as ei:
        e.boundary_points(xyz, nrm, k, float("nan"))
    assert ei.value.code == _lib.MGICP_E_INVALID
    with pytest.raises(ValueError):
        e.boundary_points(xyz, nrm[:-1], k)
    ok = _lib.MGICP_OK
    bad = _lib.MGICP_E_INVALID
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD)[0] == ok
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, stride=8)[0] == bad
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, stride=14)[0] == bad
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, nstride=8)[0] == bad
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, nstride=14)[0] == bad
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, src=False)[0] == bad
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, nsrc=False)[0] == bad
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, flags=False)[0] == bad
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, ctx=False)[0] == bad
    # n = 0 is fine, with or without pointers
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, n=0)[0] == ok
    assert _raw(e, xyz, nrm, k, bc.THRESHOLD, n=0, src=False, nsrc=False, flags=False)[0] == ok


def test_pcl_normal_records():
    """32-byte pcl::Normal input records (normal, pad, curvature, pads) and [n, 4] getNormals arrays"""
    e = _engine()
    xyz, nrm, k = bc.case("huge_radius")
    flags, gap, _nn, _ = _run("huge_radius")
    rec = np.full((len(xyz), 8), np.nan, np.float32)  # NaN everywhere but in the normals
    rec[:, :3] = nrm
    rc, f, g, _ix = _raw(e, xyz, rec, k, bc.THRESHOLD, gap=True)
    assert rc == 0 and rec.strides[0] == 32
    np.testing.assert_array_equal(f, flags)
    np.testing.assert_array_equal(_bits(g), _bits(gap))
    four = np.concatenate([nrm, np.full((len(xyz), 1), np.nan, np.float32)], 1)
    f, g, _ix, _ = e.boundary_points(xyz, four, k, bc.THRESHOLD, want_gap=True)
    np.testing.assert_array_equal(_bits(g), _bits(gap))
    # 32-byte point records too
    prec = np.full((len(xyz), 8), np.nan, np.float32)
    prec[:, :3] = xyz
    rc, f, g, _ix = _raw(e, prec, rec, k, bc.THRESHOLD, gap=True, stride=32)
    assert rc == 0
    np.testing.assert_array_equal(_bits(g), _bits(gap))


def test_set_source_and_target_survive(cube_clouds):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, _ = cube_clouds
    e = GICPEngine()
    e.set_source_xyz(src)
    e.set_target_xyz(tgt)
    T0 = e.align()
    xyz, nrm, k = bc.case("huge_radius")
    for want in (True, False):
        f, g, _ix, _ = e.boundary_points(xyz, nrm, k, bc.THRESHOLD, want_gap=True, want_indices=want)
        np.testing.assert_array_equal(_bits(g), _bits(_run("huge_radius")[1]))
    T1 = e.align()
    np.testing.assert_array_equal(_bits(T0), _bits(T1))
    e.close()


def test_obtainBoundaryKeypoints_mirror():
    from leica_point_cloud_processing_amd.cloud import PointCloudRGB
    from leica_point_cloud_processing_amd.initial_alignment import obtainBoundaryKeypoints

    xyz, nrm, k = bc.case("part")
    assert k == 30
    flags = _run("part")[0]
    status, kp, nkp = obtainBoundaryKeypoints(PointCloudRGB.from_xyz(xyz), nrm, engine=_engine())
    assert status == 0 and kp.dtype == np.int32
    np.testing.assert_array_equal(kp, np.flatnonzero(flags))
    np.testing.assert_array_equal(nkp, np.flatnonzero(~flags))
    status, kp2, _ = obtainBoundaryKeypoints(xyz, np.concatenate([nrm, nrm[:, :1]], 1), engine=_engine())
    assert status == 0
    np.testing.assert_array_equal(kp2, kp)
    # -1: normals that do not match the cloud; no keypoint found (no normal at all, or an empty cloud)
    status, kp, nkp = obtainBoundaryKeypoints(xyz, nrm[:-1], engine=_engine())
    assert status == -1 and len(kp) == 0 and len(nkp) == 0
    status, kp, nkp = obtainBoundaryKeypoints(xyz, np.full_like(nrm, np.nan), engine=_engine())
    assert status == -1 and len(kp) == 0 and len(nkp) == len(xyz)
    status, kp, nkp = obtainBoundaryKeypoints(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), engine=_engine())
    assert status == -1 and len(kp) == 0 and len(nkp) == 0


def test_adapter_obtainBoundaryKeypoints_replay(tmp_path):
    """adapter/InitialAlignment_mi355x.cpp through its C++ driver: the index lists of
    GICPEngine.boundary_points, appended to a keypoint cloud that keeps its old points."""
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_boundary")
    assert os.path.exists(exe), "build it with `make boundary-replay`"
    for name in ("part", "nonfinite"):
        xyz, nrm, k = bc.case(name)
        assert k == 30
        files = [tmp_path / f for f in ("cloud.bin", "normals.bin", "kp.bin", "nkp.bin")]
        np.ascontiguousarray(xyz, np.float32).tofile(files[0])
        np.ascontiguousarray(nrm, np.float32).tofile(files[1])
        r = subprocess.run([exe] + [str(f) for f in files], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr[-4000:]
        checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines())
                  if len(p) == 2 and p[1] in ("ok", "FAIL")}
        assert len(checks) >= 6 and all(checks.values()), checks
        flags = _run(name)[0]
        np.testing.assert_array_equal(np.fromfile(files[2], np.int32), np.flatnonzero(flags))
        np.testing.assert_array_equal(np.fromfile(files[3], np.int32), np.flatnonzero(~flags))
        assert f"keypoints {int(flags.sum())} non_keypoints {int((~flags).sum())} status 0" in r.stdout
