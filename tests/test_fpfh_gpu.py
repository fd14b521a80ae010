"""mgicp_fpfh_features (pcl::FPFHEstimation with a radius search, InitialAlignment::obtainFeatures) on the GPU
against the NumPy / SciPy reference of tests/fpfh_cases.py.

Exact where the quantity is exact: the set sizes, the records outside the union, the bin counts of every
firm row, NaN and zero histograms, the counters, the bits of a repeated call, of the calls that leave
outputs out and of permuted or repeated keypoints.  On a non-firm row each feature's count total is within
the row's number of non-firm pairs of the truth's and the L1 difference within twice that number.  A
histogram bin is held to 100 (12 m_q + 16) 2^-24 of the fp64 evaluation of the weighting formula from the
engine's own counts, and from the truth counts where every contributing row is firm.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fpfh_cases as fc
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
    """the engine's outputs for a case (every output asked for), computed once and shared"""
    if name not in _RUNS:
        xyz, nrm, kp, radius = fc.case(name)
        _RUNS[name] = _engine().fpfh_features(xyz, nrm, kp, radius, want_spfh=True)
    return _RUNS[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _raw(e, xyz, nrm, kp, radius, counts=False, sizes=False, info=False, stride=12, nstride=None, ostride=132, n=None,
         nk=None, src=True, nsrc=True, out=True, ctx=True, fill=0.0):
    """the C call itself with any of the optional outputs NULL: (status, fpfh records, counts, sizes)"""
    from leica_point_cloud_processing_amd import _lib

    n = len(xyz) if n is None else n
    nrm = np.ascontiguousarray(nrm, np.float32)
    kp = None if kp is None else np.ascontiguousarray(kp, np.int32)
    nk = (n if kp is None else len(kp)) if nk is None else nk
    o = np.full((max(nk, 1), max(ostride, 132) // 4), fill, np.float32)
    c = np.zeros((max(n, 1), 33), np.uint16)
    s = np.zeros(max(n, 1), np.int32)
    fi = _lib.MgicpFpfhInfo()
    rc = e._lib.mgicp_fpfh_features(
        e._h if ctx else None, ctypes.c_void_p(xyz.ctypes.data) if src else None, n, stride,
        ctypes.c_void_p(nrm.ctypes.data) if nsrc else None, (nrm.strides[0] if nrm.ndim == 2 and len(nrm) else 12)
        if nstride is None else nstride, ctypes.c_void_p(kp.ctypes.data) if kp is not None else None, nk,
        radius, ctypes.c_void_p(o.ctypes.data) if out else None, ostride,
        ctypes.c_void_p(c.ctypes.data) if counts else None, ctypes.c_void_p(s.ctypes.data) if sizes else None,
        ctypes.byref(fi) if info else None)
    return rc, o[:nk], c[:n], s[:n]


@pytest.mark.parametrize("name", fc.CASES)
def test_sizes_counts_and_counters(name):
    xyz, nrm, kp, radius = fc.case(name)
    ref = fc.case_reference(name)
    n = len(xyz)
    nk = n if kp is None else len(kp)
    fpfh, counts, sizes, info = _run(name)
    assert fpfh.shape == (nk, 33) and fpfh.dtype == np.float32
    assert counts.shape == (n, 33) and counts.dtype == np.uint16 and sizes.shape == (n,) and sizes.dtype == np.int32
    # sizes: the reference's, and 0 exactly on the records outside the union
    np.testing.assert_array_equal(sizes, ref.size)
    np.testing.assert_array_equal(sizes == 0, ~ref.union)
    assert not counts[~ref.union].any()
    # counts: exact on every firm row
    firm = ref.nonfirm == 0
    np.testing.assert_array_equal(counts[firm].astype(np.int64), ref.counts[firm])
    # a non-firm row: per feature the total within the number of non-firm pairs, the L1 difference within twice
    d = counts.astype(np.int64) - ref.counts
    for f in range(3):
        tot = np.abs(d[:, 11 * f:11 * f + 11].sum(1))
        l1 = np.abs(d[:, 11 * f:11 * f + 11]).sum(1)
        assert (tot <= ref.nonfirm).all() and (l1 <= 2 * ref.nonfirm).all(), (name, f, int(tot.max()), int(l1.max()))
    # a row's counts: at most one per other member and feature
    c3 = counts.astype(np.int64).reshape(n, 3, 11).sum(2)
    assert (c3 <= np.maximum(ref.size - 1, 0)[:, None]).all()
    fin = np.isfinite(xyz).all(1)
    assert info["n_finite"] == fin.sum() == ref.n_finite
    assert info["n_keypoints"] == nk
    assert info["n_nan"] == (nk - fin[np.arange(n) if kp is None else kp].sum())
    assert info["n_spfh_rows"] == ref.union.sum()
    assert info["pair_features"] <= info["pair_tests"]
    assert info["pair_features"] == c3[:, 0].sum() == c3[:, 1].sum() == c3[:, 2].sum()
    assert abs(info["pair_features"] - ref.n_features) <= ref.nonfirm.sum()
    assert info["pair_tests"] >= ref.size.sum()  # every member of a computed row was tested at least once
    assert info["ms_total"] >= info["ms_device"] >= 0 and info["ms_grid"] >= 0
    print(name, "keypoints", nk, "rows", int(info["n_spfh_rows"]), "non-firm rows", int((~firm & ref.union).sum()),
          "rows differing", int((d != 0).any(1).sum()), "pair tests", info["pair_tests"], "features",
          info["pair_features"], "largest set", int(ref.size.max(initial=0)), "ms_device", info["ms_device"])


@pytest.mark.parametrize("name", fc.CASES)
def test_histograms_within_bound(name):
    xyz, nrm, kp, radius = fc.case(name)
    ref = fc.case_reference(name)
    fpfh, counts, _sizes, _info = _run(name)
    nk = len(fpfh)
    got = fpfh.astype(np.float64)
    # against the fp64 evaluation from the engine's own counts
    hist, m, _firm, lone = fc.histograms(ref, kp, counts)
    nan = np.isnan(hist[:, 0]) if nk else np.zeros(0, bool)
    kpi = np.arange(len(xyz)) if kp is None else np.asarray(kp)
    np.testing.assert_array_equal(nan, ~np.isfinite(xyz).all(1)[kpi])
    # NaN exactly for non-finite keypoints (every bin), zeros exactly for lone ones
    np.testing.assert_array_equal(np.isnan(fpfh), np.repeat(nan[:, None], 33, 1))
    assert not _bits(fpfh[lone]).any()
    ok = ~nan
    bound = fc.hist_bound(m)[:, None]
    err = np.abs(got - hist)
    assert (err[ok] <= np.broadcast_to(bound, err.shape)[ok]).all(), (name, float(np.nanmax(err[ok] / bound[ok])))
    # on keypoints whose contributing rows are all firm: the same bound against the truth counts
    thist, tm, tfirm, tlone = fc.case_histograms(name)
    np.testing.assert_array_equal(tm, m)
    np.testing.assert_array_equal(tlone, lone)
    sel = ok & tfirm
    terr = np.abs(got - thist)
    assert (terr[sel] <= np.broadcast_to(bound, terr.shape)[sel]).all(), (name, float(np.nanmax(terr[sel] / bound[sel])))
    # each feature's bins sum to 100 within the bound or are all 0
    for f in range(3):
        blk = got[:, 11 * f:11 * f + 11]
        s = blk.sum(1)
        zero = (blk == 0).all(1)
        assert (zero[ok] | (np.abs(s - 100.0) <= bound[:, 0])[ok]).all(), (name, f)
    assert (got[ok] >= 0).all()
    if ok.any():
        print(name, "largest error / bound", float((err[ok] / bound[ok]).max()), "vs truth counts",
              float((terr[sel] / bound[sel]).max()) if sel.any() else None, "firm keypoints", int(sel.sum()), "of", int(ok.sum()),
              "lone", int(lone.sum()))


@pytest.mark.parametrize("name", ("part_kp", "clump", "nonfinite", "dups", "radius_zero", "n0", "n2"))
def test_repeatable_and_optional_outputs(name):
    e = _engine()
    xyz, nrm, kp, radius = fc.case(name)
    fpfh, counts, sizes, info = _run(name)
    # a repeated call gives the same bits in every output
    f2, c2, s2, info2 = e.fpfh_features(xyz, nrm, kp, radius, want_spfh=True)
    np.testing.assert_array_equal(_bits(f2), _bits(fpfh))
    np.testing.assert_array_equal(c2, counts)
    np.testing.assert_array_equal(s2, sizes)
    for key in ("n_finite", "n_keypoints", "n_nan", "n_spfh_rows", "pair_tests", "pair_features"):
        assert info2[key] == info[key], key
    # spfh_counts, spfh_sizes and info NULL, one at a time and all together
    for kw in ({"counts": True, "sizes": True}, {"sizes": True, "info": True}, {"counts": True, "info": True}, {}):
        rc, f3, c3, s3 = _raw(e, xyz, nrm, kp, radius, **kw)
        assert rc == 0
        np.testing.assert_array_equal(_bits(f3[:, :33]), _bits(fpfh), err_msg=str(kw))
        if kw.get("counts"):
            np.testing.assert_array_equal(c3, counts)
        if kw.get("sizes"):
            np.testing.assert_array_equal(s3, sizes)


def test_null_keypoints_equal_arange():
    e = _engine()
    xyz, nrm, kp, radius = fc.case("part_all")
    assert kp is None
    fpfh, counts, sizes, _ = _run("part_all")
    f2, c2, s2, _ = e.fpfh_features(xyz, nrm, np.arange(len(xyz), dtype=np.int32), radius, want_spfh=True)
    np.testing.assert_array_equal(_bits(f2), _bits(fpfh))
    np.testing.assert_array_equal(c2, counts)
    np.testing.assert_array_equal(s2, sizes)


def test_permuted_and_repeated_keypoints():
    """`shuffled` holds the keypoints of `part_3res` in another order, a third of them twice: the same rows"""
    xyz, nrm, kp, radius = fc.case("part_3res")
    _x, _n, kp2, radius2 = fc.case("shuffled")
    assert radius2 == radius and len(kp2) > len(kp) and set(kp2.tolist()) == set(kp.tolist())
    fpfh, counts, sizes, _ = _run("part_3res")
    f2, c2, s2, info2 = _run("shuffled")
    where = {int(k): i for i, k in enumerate(kp)}
    rows = np.array([where[int(k)] for k in kp2])
    np.testing.assert_array_equal(_bits(f2), _bits(fpfh[rows]))
    np.testing.assert_array_equal(c2, counts)
    np.testing.assert_array_equal(s2, sizes)
    assert info2["n_keypoints"] == len(kp2)


def test_records_and_strides():
    """32-byte point and pcl::Normal records; a wider output stride leaves the other bytes untouched"""
    e = _engine()
    xyz, nrm, kp, radius = fc.case("nonfinite")
    fpfh, counts, sizes, _ = _run("nonfinite")
    prec = np.full((len(xyz), 8), np.nan, np.float32)
    prec[:, :3] = xyz
    nrec = np.full((len(xyz), 8), np.nan, np.float32)
    nrec[:, :3] = nrm
    rc, f, c, s = _raw(e, prec, nrec, kp, radius, counts=True, sizes=True, stride=32)
    assert rc == 0 and nrec.strides[0] == 32
    np.testing.assert_array_equal(_bits(f[:, :33]), _bits(fpfh))
    np.testing.assert_array_equal(c, counts)
    np.testing.assert_array_equal(s, sizes)
    four = np.concatenate([nrm, np.full((len(xyz), 1), np.nan, np.float32)], 1)
    f4, _c, _s, _ = e.fpfh_features(xyz, four, kp, radius)
    np.testing.assert_array_equal(_bits(f4), _bits(fpfh))
    for ostride in (132, 136, 160):
        rc, f, _c, _s = _raw(e, xyz, nrm, kp, radius, ostride=ostride, fill=-7.0)
        assert rc == 0 and f.shape[1] == ostride // 4
        np.testing.assert_array_equal(_bits(f[:, :33]), _bits(fpfh))
        assert (f[:, 33:] == -7.0).all()


def test_dropping_nonfinite_records_gives_the_same_bits():
    e = _engine()
    xyz, nrm, kp, radius = fc.case("nonfinite")
    fpfh, counts, sizes, _ = _run("nonfinite")
    fin = np.isfinite(xyz).all(1)
    new = np.cumsum(fin) - 1
    keep = fin[kp]
    f2, c2, s2, info = e.fpfh_features(np.ascontiguousarray(xyz[fin]), np.ascontiguousarray(nrm[fin]),
                                       new[kp[keep]].astype(np.int32), radius, want_spfh=True)
    np.testing.assert_array_equal(_bits(f2), _bits(fpfh[keep]))
    np.testing.assert_array_equal(c2, counts[fin])
    np.testing.assert_array_equal(s2, sizes[fin])
    assert info["n_nan"] == 0 and not counts[~fin].any() and not sizes[~fin].any()


def test_invalid_arguments():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    xyz, nrm, kp, radius = fc.case("huge_radius")
    n = len(xyz)
    ok, bad = _lib.MGICP_OK, _lib.MGICP_E_INVALID
    for bad_kp in ([0, n], [-1, 3], [5, 2 ** 31 - 1]):
        with pytest.raises(_lib.MgicpError) as ei:
            e.fpfh_features(xyz, nrm, np.array(bad_kp, np.int32), radius)
        assert ei.value.code == bad
    for bad_radius in (-0.1, float("nan")):
        with pytest.raises(_lib.MgicpError) as ei:
            e.fpfh_features(xyz, nrm, kp, bad_radius)
        assert ei.value.code == bad
    with pytest.raises(ValueError):
        e.fpfh_features(xyz, nrm[:-1], kp, radius)
    assert _raw(e, xyz, nrm, kp, radius)[0] == ok
    for kw in ({"stride": 8}, {"stride": 14}, {"nstride": 8}, {"nstride": 14}, {"ostride": 128}, {"ostride": 134},
               {"src": False}, {"nsrc": False}, {"out": False}, {"ctx": False}):
        assert _raw(e, xyz, nrm, kp, radius, **kw)[0] == bad, kw
    # n = 0 or no keypoint is fine, with or without pointers
    assert _raw(e, xyz, nrm, kp, radius, n=0, nk=0)[0] == ok
    assert _raw(e, xyz, nrm, None, radius, n=0, src=False, nsrc=False, out=False)[0] == ok
    rc, _f, c, s = _raw(e, xyz, nrm, kp, radius, nk=0, out=False, counts=True, sizes=True)
    assert rc == ok and not c.any() and not s.any()


def test_set_larger_than_the_limit_is_refused():
    """70000 records within one radius: a set above 65535, refused with a message that names the limit"""
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    rng = np.random.default_rng(31)
    xyz = rng.uniform(0, 0.01, (70000, 3)).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(xyz), 1))
    with pytest.raises(_lib.MgicpError) as ei:
        e.fpfh_features(xyz, nrm, np.array([5], np.int32), 1.0)
    assert ei.value.code == _lib.MGICP_E_INVALID and str(fc.MAX_SET) in str(ei.value)
    # the engine still serves the next call
    fpfh, _c, _s, _ = e.fpfh_features(*fc.case("n3"))
    np.testing.assert_array_equal(_bits(fpfh), _bits(_run("n3")[0]))


def test_set_source_and_target_survive(cube_clouds):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, _ = cube_clouds
    e = GICPEngine()
    e.set_source_xyz(src)
    e.set_target_xyz(tgt)
    T0 = e.align()
    xyz, nrm, kp, radius = fc.case("huge_radius")
    for want in (True, False):
        f, _c, _s, _ = e.fpfh_features(xyz, nrm, kp, radius, want_spfh=want)
        np.testing.assert_array_equal(_bits(f), _bits(_run("huge_radius")[0]))
    T1 = e.align()
    np.testing.assert_array_equal(_bits(T0), _bits(T1))
    e.close()


def test_obtainFeatures_mirror():
    from leica_point_cloud_processing_amd.cloud import PointCloudRGB
    from leica_point_cloud_processing_amd.initial_alignment import RADIUS_FACTOR, obtainFeatures

    e = _engine()
    xyz, nrm, kp, _radius = fc.case("part_kp")
    assert RADIUS_FACTOR == 1.4
    want, _c, _s, _ = e.fpfh_features(xyz, nrm, kp, e.cloud_resolution(xyz) * 1.4)
    status, feats = obtainFeatures(PointCloudRGB.from_xyz(xyz), nrm, kp, engine=e)
    assert status == 0 and feats.dtype == np.float32 and feats.shape == (len(kp), 33)
    np.testing.assert_array_equal(_bits(feats), _bits(want))
    status, feats4 = obtainFeatures(xyz, np.concatenate([nrm, nrm[:, :1]], 1), kp, engine=e)
    assert status == 0
    np.testing.assert_array_equal(_bits(feats4), _bits(want))
    want3, _c, _s, _ = e.fpfh_features(xyz, nrm, kp, e.cloud_resolution(xyz) * 3.0)
    status, feats3 = obtainFeatures(xyz, nrm, kp, radius_factor=3.0, engine=e)
    np.testing.assert_array_equal(_bits(feats3), _bits(want3))
    assert (feats3 != feats).any()
    # -1: no feature comes back (no keypoint; normals that do not match the cloud)
    status, none = obtainFeatures(xyz, nrm, np.zeros(0, np.int32), engine=e)
    assert status == -1 and none.shape == (0, 33)
    status, none = obtainFeatures(xyz, nrm[:-1], kp, engine=e)
    assert status == -1 and none.shape == (0, 33)


def test_adapter_obtainFeatures_replay(tmp_path):
    """adapter/InitialAlignment_mi355x.cpp through its C++ driver: the FPFHSignature33 records of
    GICPEngine.fpfh_features at the resolution-derived radius."""
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_fpfh")
    assert os.path.exists(exe), "build it with `make fpfh-replay`"
    e = _engine()
    for name in ("part_kp", "nonfinite"):
        xyz, nrm, kp, _radius = fc.case(name)
        files = [tmp_path / f for f in ("cloud.bin", "normals.bin", "kp.bin", "fpfh.bin")]
        np.ascontiguousarray(xyz, np.float32).tofile(files[0])
        np.ascontiguousarray(nrm, np.float32).tofile(files[1])
        np.ascontiguousarray(kp, np.int32).tofile(files[2])
        r = subprocess.run([exe] + [str(f) for f in files], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr[-4000:]
        checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines())
                  if len(p) == 2 and p[1] in ("ok", "FAIL")}
        assert len(checks) >= 4 and all(checks.values()), checks
        want, _c, _s, _ = e.fpfh_features(xyz, nrm, kp, e.cloud_resolution(xyz) * 1.4)
        got = np.fromfile(files[3], np.float32).reshape(-1, 33)
        np.testing.assert_array_equal(_bits(got), _bits(want))
        assert f"features {len(kp)} status 0" in r.stdout
