"""mgicp_match_features (pcl::registration::CorrespondenceEstimation over FPFHSignature33,
InitialAlignment::obtainCorrespondences) on the GPU against the NumPy reference of tests/match_cases.py.

Everything is exact: the matches, the bits of the distances, NaN exactly where there is no match, the
counters, the bits of a repeated call, of the calls that leave outputs out, of wider records, of a search split
over several launches.  No test here has a tolerance.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fpfh_cases as fc
import match_cases as mc
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
    """the engine's outputs for a case, computed once and shared: (match, distance, info)"""
    if name not in _RUNS:
        S, T, md = mc.case(name)
        _RUNS[name] = _engine().match_features(S, T, md)
    return _RUNS[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _records(X, stride):
    """the rows of X in records of `stride` bytes, the floats between them NaN"""
    rec = np.full((max(len(X), 1), stride // 4), np.nan, np.float32)
    rec[:len(X), :33] = X
    return rec


def _raw(e, S, T, md=None, dist=True, count=True, info=True, sstride=132, tstride=132, ns=None, nt=None, src=True,
         tgt=True, out=True, ctx=True):
    """the C call itself with any of the optional outputs NULL: (status, match, distance, count, info)"""
    from leica_point_cloud_processing_amd import _lib

    ns = len(S) if ns is None else ns
    nt = len(T) if nt is None else nt
    srec = _records(S, max(sstride, 132))
    trec = _records(T, max(tstride, 132))
    m = np.full(max(ns, 1), -7, np.int32)
    d = np.full(max(ns, 1), -7.0, np.float32)
    c = ctypes.c_size_t(12345)
    mi = _lib.MgicpMatchInfo()
    rc = e._lib.mgicp_match_features(
        e._h if ctx else None, ctypes.c_void_p(srec.ctypes.data) if src else None, ns, sstride,
        ctypes.c_void_p(trec.ctypes.data) if tgt else None, nt, tstride, mc.DBL_MAX if md is None else md,
        ctypes.c_void_p(m.ctypes.data) if out else None, ctypes.c_void_p(d.ctypes.data) if dist else None,
        ctypes.byref(c) if count else None, ctypes.byref(mi) if info else None)
    return rc, m[:ns], d[:ns], int(c.value), {f: getattr(mi, f) for f, _ in mi._fields_}


def _check_against(ref, match, dist, info, what):
    np.testing.assert_array_equal(match, ref.match, err_msg=what)
    np.testing.assert_array_equal(np.isnan(dist), ref.match < 0, err_msg=what)
    got = ref.match >= 0
    np.testing.assert_array_equal(_bits(dist[got]), _bits(ref.distance[got]), err_msg=what)
    assert info["n_source_valid"] == ref.n_source_valid and info["n_target_valid"] == ref.n_target_valid, what
    assert info["n_correspondences"] == ref.n_correspondences and info["n_tied"] == ref.n_tied, what
    if ref.n_target_valid:
        assert info["pair_tests"] >= ref.n_source_valid, what
    assert info["pair_tests"] <= ref.n_source_valid * ref.n_target_valid, what
    assert info["ms_total"] >= info["ms_device"] >= 0, what


@pytest.mark.parametrize("name", mc.CASES)
def test_match_distance_and_counters(name):
    S, T, _md = mc.case(name)
    ref = mc.case_reference(name)
    match, dist, info = _run(name)
    assert match.dtype == np.int32 and match.shape == (len(S),) and dist.dtype == np.float32 and dist.shape == (len(S),)
    print(name, "ns", len(S), "nt", len(T), "matched", int(info["n_correspondences"]), "tied", int(info["n_tied"]),
          "pair tests", info["pair_tests"], "ms_device", info["ms_device"], _engine().match_stats())
    _check_against(ref, match, dist, info, name)


def test_engine_fpfh_rows():
    """3res_vs_kp on the engine's own descriptors of those cases (float rows, no longer the fp64 evaluation)"""
    e = _engine()
    feats = {}
    for name in ("part_3res", "part_kp"):
        xyz, nrm, kp, radius = fc.case(name)
        feats[name] = e.fpfh_features(xyz, nrm, kp, radius)[0]
    S, T = feats["part_3res"], feats["part_kp"]
    assert S.shape == T.shape == (2069, 33)
    match, dist, info = e.match_features(S, T)
    _check_against(mc.reference(S, T), match, dist, info, "engine rows")
    assert info["n_correspondences"] == 2069


@pytest.mark.parametrize("name", ("kp_vs_kp", "nonfinite_target_nan", "sizes_65_1025", "multi_block", "huge",
                                  "all_target_nan", "maxdist_at"))
def test_repeatable_and_optional_outputs(name):
    e = _engine()
    S, T, md = mc.case(name)
    match, dist, info = _run(name)
    m2, d2, info2 = e.match_features(S, T, md)
    np.testing.assert_array_equal(m2, match)
    np.testing.assert_array_equal(_bits(d2), _bits(dist))
    for key in ("n_source_valid", "n_target_valid", "n_correspondences", "n_tied", "pair_tests"):
        assert info2[key] == info[key], key
    # distance, n_correspondences and info NULL, one at a time and all together
    for kw in ({"dist": False}, {"count": False}, {"info": False}, {"dist": False, "count": False, "info": False}):
        rc, m3, d3, c3, i3 = _raw(e, S, T, md, **kw)
        assert rc == 0, kw
        np.testing.assert_array_equal(m3, match, err_msg=str(kw))
        if kw.get("dist", True):
            np.testing.assert_array_equal(_bits(d3), _bits(dist), err_msg=str(kw))
        else:
            assert (d3 == -7.0).all()
        assert c3 == (info["n_correspondences"] if kw.get("count", True) else 12345)
        if kw.get("info", True):
            assert i3["n_tied"] == info["n_tied"] and i3["n_correspondences"] == info["n_correspondences"]


def test_record_strides():
    """rows of 132, 136 and 160 bytes give the same bits; the floats between the rows are NaN, so a kernel or a
    packing loop that read them as data would lose rows"""
    e = _engine()
    S, T, md = mc.case("nonfinite_target_nan")
    match, dist, info = _run("nonfinite_target_nan")
    for sstride, tstride in ((132, 132), (136, 136), (160, 160), (132, 160), (136, 132)):
        rc, m, d, c, i = _raw(e, S, T, md, sstride=sstride, tstride=tstride)
        assert rc == 0
        np.testing.assert_array_equal(m, match, err_msg=str((sstride, tstride)))
        np.testing.assert_array_equal(_bits(d), _bits(dist))
        assert c == info["n_correspondences"] and i["n_target_valid"] == info["n_target_valid"]
    # the Python entry passes wider rows with their stride
    wide = np.full((len(S), 40), np.nan, np.float32)
    wide[:, :33] = S
    m, d, _ = e.match_features(wide, T, md)
    np.testing.assert_array_equal(m, match)
    np.testing.assert_array_equal(_bits(d), _bits(dist))
    with pytest.raises(ValueError):
        e.match_features(S[:, :32], T)
    with pytest.raises(ValueError):
        e.match_features(S, T.reshape(-1))


@pytest.mark.parametrize("name", ("kp_vs_kp", "3res_vs_kp", "multi_block"))
def test_permuted_target(name):
    e = _engine()
    S, T, md = mc.case(name)
    ref = mc.case_reference(name)
    match, dist, info = _run(name)
    perm = np.random.default_rng(51).permutation(len(T))     # row k of the permuted target is row perm[k]
    m2, d2, info2 = e.match_features(S, np.ascontiguousarray(T[perm]), md)
    np.testing.assert_array_equal(_bits(d2), _bits(dist))
    assert info2["n_tied"] == info["n_tied"] and info2["n_correspondences"] == info["n_correspondences"]
    free = ~ref.tied
    np.testing.assert_array_equal(perm[m2[free]], match[free])
    # a tied query: some row with the same distance, and the lowest such row of the permuted target
    tied = np.flatnonzero(ref.tied)
    if len(tied):
        D = mc.d2_matrix(S[tied], T[perm])
        np.testing.assert_array_equal(m2[tied], (D == dist[tied][:, None]).argmax(1))


def test_dropping_nan_targets_gives_the_same_matches():
    e = _engine()
    S, T, md = mc.case("nonfinite_target_nan")
    match, dist, info = _run("nonfinite_target_nan")
    ok = np.isfinite(T).all(1)
    new = np.cumsum(ok) - 1
    m2, d2, info2 = e.match_features(S, np.ascontiguousarray(T[ok]), md)
    got = match >= 0
    np.testing.assert_array_equal(m2 >= 0, got)
    np.testing.assert_array_equal(m2[got], new[match[got]])
    np.testing.assert_array_equal(_bits(d2), _bits(dist))
    assert info2["n_target_valid"] == info["n_target_valid"] == ok.sum() and info2["n_tied"] == info["n_tied"]


def test_winner_positions():
    """one query, the unique winner at the ends, at the wave's edge and just either side of the edges between
    the blocks that share a launch's targets and between the launches"""
    from leica_point_cloud_processing_amd.engine import GICPEngine

    e = GICPEngine(options={"match_pairs_per_launch": 4096})
    nt = 10007
    q, T = mc.winner_case(nt, 0)
    e.match_features(q, T)
    st = e.match_stats()
    print(st)
    per_launch, per_split = st["rows_per_launch"], st["rows_per_split"]
    assert per_launch == 4096 and st["launches"] == 3 and st["splits"] > 1 and per_split * st["splits"] >= per_launch
    assert per_split < per_launch < nt
    positions = [0, 63, 64, nt - 1, per_split - 1, per_split, per_launch - per_split - 1, per_launch - 1, per_launch,
                 2 * per_launch - 1, 2 * per_launch, 2 * per_launch + per_split - 1, 2 * per_launch + per_split]
    for pos in positions:
        q, T = mc.winner_case(nt, pos)
        match, dist, info = e.match_features(q, T)
        assert match.tolist() == [pos] and info["n_tied"] == 0, pos
        assert _bits(dist).tolist() == _bits(mc.reference(q, T).distance).tolist()
    # a second copy of the winner in another launch: tied, the lower row wins
    for a, b in ((5, 2 * per_launch + 7), (per_launch - 1, per_launch), (per_split - 1, per_split)):
        q, T = mc.winner_case(nt, a)
        T[b] = T[a]
        match, _d, info = e.match_features(q, T)
        assert match.tolist() == [a] and info["n_tied"] == 1, (a, b)
    e.close()


def test_launch_split_gives_the_same_bits():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    for name, pairs in (("multi_block", 4099 * 1000), ("kp_vs_kp", 2069 * 100), ("late_bins", mc.LATE_NS * 64)):
        S, T, md = mc.case(name)
        match, dist, info = _run(name)
        e = GICPEngine(options={"match_pairs_per_launch": pairs})
        m2, d2, info2 = e.match_features(S, T, md)
        st = e.match_stats()
        print(name, st)
        assert st["launches"] >= 10 and st["pairs"] == info["pair_tests"]
        assert 0 <= st["left_after_8"] + st["left_after_16"] + st["left_after_24"] <= st["pairs"]
        np.testing.assert_array_equal(m2, match)
        np.testing.assert_array_equal(_bits(d2), _bits(dist))
        assert info2["n_tied"] == info["n_tied"] and info2["pair_tests"] == info["pair_tests"]
        e.debug_option("match_pairs_per_launch", 0)     # back to the default: one launch at these sizes
        m3, d3, _ = e.match_features(S, T, md)
        assert e.match_stats()["launches"] == 1
        np.testing.assert_array_equal(m3, match)
        np.testing.assert_array_equal(_bits(d3), _bits(dist))
        e.close()


def test_invalid_arguments():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    S, T, _ = mc.case("sizes_65_1025")
    ok, bad = _lib.MGICP_OK, _lib.MGICP_E_INVALID
    assert _raw(e, S, T)[0] == ok
    for kw in ({"sstride": 128}, {"sstride": 134}, {"tstride": 128}, {"tstride": 134}, {"ctx": False}, {"src": False},
               {"tgt": False}, {"out": False}, {"md": -0.5}, {"md": float("nan")}, {"md": -float("inf")}):
        assert _raw(e, S, T, **kw)[0] == bad, kw
    for md in (-1.0, float("nan")):
        with pytest.raises(_lib.MgicpError) as ei:
            e.match_features(S, T, md)
        assert ei.value.code == bad
    # zero sizes are fine, with or without pointers
    rc, m, d, c, i = _raw(e, S, T, ns=0, src=False, out=False, dist=False)
    assert rc == ok and c == 0 and i["n_correspondences"] == 0 and i["n_source_valid"] == 0
    assert i["n_target_valid"] == len(T) and i["pair_tests"] == 0
    rc, m, d, c, i = _raw(e, S, T, nt=0, tgt=False)
    assert rc == ok and c == 0 and (m == -1).all() and np.isnan(d).all() and i["n_source_valid"] == len(S)
    assert _raw(e, S, T, ns=0, nt=0, src=False, tgt=False, out=False, dist=False, count=False, info=False)[0] == ok
    # max_distance = +inf rejects nothing, like DBL_MAX
    rc, m, d, c, i = _raw(e, S, T, md=float("inf"))
    assert rc == ok
    np.testing.assert_array_equal(m, mc.case_reference("sizes_65_1025").match)


def test_set_source_and_target_survive(cube_clouds):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, _ = cube_clouds
    e = GICPEngine()
    e.set_source_xyz(src)
    e.set_target_xyz(tgt)
    T0 = e.align()
    S, T, md = mc.case("sizes_257_4099")
    m, d, _ = e.match_features(S, T, md)
    np.testing.assert_array_equal(m, mc.case_reference("sizes_257_4099").match)
    T1 = e.align()
    np.testing.assert_array_equal(_bits(T0), _bits(T1))
    e.close()


def test_obtainCorrespondences_mirror():
    from leica_point_cloud_processing_amd.initial_alignment import obtainCorrespondences

    e = _engine()
    for name in ("nonfinite_target_nan", "kp_vs_3res", "all_target_nan"):
        S, T, _ = mc.case(name)
        ref = mc.case_reference(name)
        iq, im, dist = obtainCorrespondences(S, T, engine=e)
        assert iq.dtype == np.int32 and im.dtype == np.int32 and dist.dtype == np.float32
        want = np.flatnonzero(ref.match >= 0)
        np.testing.assert_array_equal(iq, want)          # compacted, ascending index_query
        np.testing.assert_array_equal(im, ref.match[want])
        np.testing.assert_array_equal(_bits(dist), _bits(ref.distance[want]))
    assert len(mc.case_reference("nonfinite_target_nan").match) > len(obtainCorrespondences(*mc.case("nonfinite_target_nan")[:2], engine=e)[0]) > 0


def test_adapter_obtainCorrespondences_replay(tmp_path):
    """adapter/InitialAlignment_mi355x.cpp through its C++ driver: the pcl::Correspondences of
    GICPEngine.match_features, compacted in ascending index_query."""
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_correspondences")
    assert os.path.exists(exe), "build it with `make corr-replay`"
    for name in ("kp_vs_3res", "nonfinite"):
        S, T, _ = mc.case(name)
        match, dist, _info = _run(name)
        files = [tmp_path / f for f in ("source.bin", "target.bin", "query.bin", "match.bin", "distance.bin")]
        np.ascontiguousarray(S, np.float32).tofile(files[0])
        np.ascontiguousarray(T, np.float32).tofile(files[1])
        r = subprocess.run([exe] + [str(f) for f in files], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr[-4000:]
        checks = {p[0]: p[1] == "ok" for p in (line.split() for line in r.stdout.splitlines())
                  if len(p) == 2 and p[1] in ("ok", "FAIL")}
        assert len(checks) >= 5 and all(checks.values()), checks
        want = np.flatnonzero(match >= 0)
        np.testing.assert_array_equal(np.fromfile(files[2], np.int32), want)
        np.testing.assert_array_equal(np.fromfile(files[3], np.int32), match[want])
        np.testing.assert_array_equal(_bits(np.fromfile(files[4], np.float32)), _bits(dist[want]))
        assert f"correspondences {len(want)}" in r.stdout and f"Found {len(want)} correspondences" in r.stdout + r.stderr
