"""CPU tests of the FPFH cases (tests/fpfh_cases.py): every cloud is what it claims to be, the share of
non-firm rows stays under the cap in every case (a condition on the inputs, not a tolerance on the engine),
and the float32 model of the specified arithmetic gives the truth bins on every firm pair -- so TOL is about
the arithmetic, not about the engine.  Also: the adapter compiles against its stand-ins, and the ctypes
mirror matches the header."""
import os
import subprocess

import numpy as np
import pytest

import boundary_cases as bc
import fpfh_cases as fc
import normals_cases as nc
from cluster_edges_cases import d2_f32, r2_of
from conftest import ROOT


@pytest.mark.parametrize("name", fc.CASES)
def test_reference_shapes_and_sets(name):
    xyz, nrm, kp, radius = fc.case(name)
    ref = fc.case_reference(name)
    n = len(xyz)
    assert xyz.dtype == np.float32 and xyz.shape == (n, 3) and nrm.dtype == np.float32 and nrm.shape == (n, 3)
    assert kp is None or (kp.dtype == np.int32 and kp.ndim == 1 and ((kp >= 0) & (kp < n)).all())
    fin = np.isfinite(xyz).all(1)
    np.testing.assert_array_equal(ref.finite, fin)
    assert ref.n_finite == fin.sum()
    assert ref.counts.shape == (n, 33) and ref.size.shape == (n,)
    # the sets by brute force on the small cases: float d2 < float(radius^2), strict, finite records only
    if 0 < n <= 1000:
        r2 = r2_of(radius)
        pts = xyz[fin]
        d2 = d2_f32(pts[:, None, :], pts[None, :, :])
        member = d2 < r2
        np.testing.assert_array_equal(ref.full_size[fin], member.sum(1))
        kpf = np.zeros(len(pts), bool)
        kpi = np.arange(n) if kp is None else kp
        kpf[ref.pos[kpi[fin[kpi]]]] = True
        np.testing.assert_array_equal(ref.union[fin], member[kpf].any(0))
    assert not ref.union[~fin].any() and (ref.size[~ref.union] == 0).all() and not ref.counts[~ref.union].any()
    if r2_of(radius) > 0:
        assert (ref.size[ref.union] >= 1).all()
        kpi = np.arange(n) if kp is None else kp
        assert ref.union[kpi[fin[kpi]]].all()  # a finite keypoint is in its own set
    # one count per feature and valid pair; never more than the other members
    c3 = ref.counts.reshape(n, 3, 11).sum(2)
    assert (c3[:, 0] == c3[:, 1]).all() and (c3[:, 1] == c3[:, 2]).all()
    assert (c3[:, 0] <= np.maximum(ref.size - 1, 0)).all() and c3[:, 0].sum() == ref.n_features
    assert (ref.nonfirm <= np.maximum(ref.size - 1, 0)).all()


def test_cases_are_what_they_claim():
    # part_kp: the reference's setting -- about 1.5 neighbours on average and many lone keypoints
    xyz, nrm, kp, radius = fc.case("part_kp")
    ref = fc.case_reference("part_kp")
    _h, _m, _firm, lone = fc.case_histograms("part_kp")
    _scan, res = nc._part_scan()
    assert radius == 1.4 * res and 500 <= len(kp) <= 3000 and np.isfinite(nrm[kp]).all()
    mean = ref.full_size[kp].mean() - 1
    print("part_kp keypoints", len(kp), "mean neighbours", mean, "lone", int(lone.sum()))
    assert 0.5 <= mean <= 3.0 and lone.sum() >= 100
    assert fc.case("part_3res")[3] == 3.0 * res and fc.case("part_all")[2] is None
    assert (fc.case("part_3res")[2] == kp).all()
    # cube: unit face normals; thousands of exact a1 = a2 ties between two branches with equal bins
    xyz, nrm, kp, radius = fc.case("cube")
    ref = fc.case_reference("cube")
    assert kp is None and (np.abs(nrm).sum(1) == 1).all() and len(np.unique(nrm, axis=0)) == 6
    pts = xyz.astype(np.float64)
    dp = pts[ref.pair_J] - pts[ref.pair_I]
    a1 = (nrm[ref.pair_I] * dp).sum(1)
    a2 = (nrm[ref.pair_J] * dp).sum(1)
    ties = int((np.abs(a1) == np.abs(a2)).sum())
    print("cube pairs", len(a1), "exact ties", ties)
    assert ties >= 5000 and ref.pair_firm[np.abs(a1) == np.abs(a2)].all()
    # clump: sets above 255 and above a wave's lanes; huge_radius: every finite record in every set
    ref = fc.case_reference("clump")
    assert ref.size.max() > 255 and (ref.size > 64).sum() >= 1000 and (ref.size == 1).sum() >= 1000
    xyz, nrm, kp, radius = fc.case("huge_radius")
    ref = fc.case_reference("huge_radius")
    assert len(xyz) == 777 and (ref.size == 777).all() and len(kp) == 111
    g, _keys, counts = __import__("cluster_edges_cases").cell_counts(xyz, 2.0 * radius)
    assert list(g.dims) == [1, 1, 1] and counts.max() == 777
    # nonfinite: non-finite records and NaN normals, some of each among the keypoints
    xyz, nrm, kp, radius = fc.case("nonfinite")
    fin = np.isfinite(xyz).all(1)
    has = np.isfinite(nrm).all(1)
    assert (~fin).sum() == 50 and (~fin[kp]).sum() >= 20 and (fin[kp] & ~has[kp]).sum() >= 20
    assert np.isnan(xyz).any() and np.isinf(xyz).any() and np.isnan(nrm[fin]).any() and np.isinf(nrm[fin]).any()
    h, _m, _firm, _lone = fc.case_histograms("nonfinite")
    np.testing.assert_array_equal(np.isnan(h[:, 0]), ~fin[kp])
    # dups: every point three times -- f4 = 0 pairs and d2 = 0 members
    xyz, nrm, kp, radius = fc.case("dups")
    ref = fc.case_reference("dups")
    _u, cnt = np.unique(xyz, axis=0, return_counts=True)
    assert (cnt == 3).all()
    assert ((ref.d2 == 0) & (ref.I != ref.J)).sum() == 2 * len(xyz)
    same = (xyz[ref.fin_idx][ref.pair_I] == xyz[ref.fin_idx][ref.pair_J]).all(1)
    assert same.sum() == 2 * len(xyz) and not ref.pair_valid[same].any()
    # shuffled: the keypoints of part_3res, unsorted, some twice
    kp3 = fc.case("part_3res")[2]
    kps = fc.case("shuffled")[2]
    assert set(kps.tolist()) == set(kp3.tolist()) and len(kps) > len(kp3) and (np.diff(kps) < 0).any()
    # radius 0 links nothing; n = 0 .. 3
    assert fc.case_reference("radius_zero").union.sum() == 0
    for k in range(4):
        assert len(fc.case(f"n{k}")[0]) == k
    assert (fc.case_reference("n3").size == 3).all()


def test_far_cases_are_what_they_claim():
    assert fc.CLOUD_CASES + fc.EDGE_VALUE_CASES == fc.CASES and set(fc.FAR_CASES) <= set(fc.CLOUD_CASES)
    assert not set(fc.EDGE_VALUE_CASES) & set(fc.CLOUD_CASES) and len(fc.CLOUD_CASES) == 9 + len(fc.FAR_CASES)
    # far_sheet: the normals' radius, every fifth record a keypoint; at |X0| = 4096.5 the cell box of at least
    # a third of the records -- of the keypoints (mark, final) and of the computed rows (SPFH) alike -- has
    # more than 64 rows of cells: fpfh_walk's outer loop takes a second turn.  The control has no box above
    # 4 x 4 rows.  Conditions on the inputs from the float32 restatement of the cell function
    for name in nc.FAR_SHEET_X0:
        xyz, nrm, kp, radius = fc.case(name)
        ref = fc.case_reference(name)
        assert radius == nc.FAR_SHEET_RADIUS and (kp == np.arange(0, 6000, 5)).all() and np.isfinite(nrm).all()
        assert (xyz == nc.case(name)[0]).all() and (nrm == bc.case(name)[1]).all()
        rows, _pts, rel = nc.box_facts(xyz, radius)
        print(name, "rx / h", rel, "rows of a keypoint's box: above 64", int((rows[kp] > 64).sum()), "of", len(kp),
              "of a computed row's", int((rows[ref.union] > 64).sum()), "of", int(ref.union.sum()), "max", int(rows.max()))
        if name == "far_sheet_origin":
            assert rows.max() <= 16
        else:
            assert (rows[kp] > 64).sum() * 3 >= len(kp) and (rows[ref.union] > 64).sum() * 3 >= ref.union.sum()
            assert rows.max() > 64 and ref.size.max() <= 64  # many rows, few members: the rows are the load
    # far_part: _part()'s recipe in the site frame -- truth normals, the truth boundary keypoints of that frame
    for name, (which, factor) in fc.FAR_PART_CASES.items():
        xyz, nrm, kp, radius = fc.case(name)
        bref = bc.case_reference(which)
        assert (xyz == nc.case(which)[0]).all() and (nrm == bc.case(which)[1]).all()
        assert radius == factor * nc._far_part_base()[1] and nc.case(which)[1] == 10.0 * nc._far_part_base()[1]
        with np.errstate(invalid="ignore"):
            assert (kp == np.flatnonzero(bref.decided & (bref.truth > np.float64(np.float32(bc.THRESHOLD))))).all()
        assert 300 <= len(kp) <= 2000 and np.isfinite(nrm[kp]).all()
    # lattice_rim: sizes decided at the rim -- the reference's are the strict integer counts
    from scipy.spatial import cKDTree

    xyz, nrm, kp, radius = fc.case("lattice_rim")
    ref = fc.case_reference("lattice_rim")
    ij = nc.lattice_rim_ij()
    pairs = cKDTree(ij).query_pairs(np.sqrt(25.5), output_type="ndarray")
    d2i = ((ij[pairs[:, 0]] - ij[pairs[:, 1]]) ** 2).sum(1)
    np.testing.assert_array_equal(ref.full_size, 1 + np.bincount(pairs[d2i < 25].ravel(), minlength=len(ij)))
    assert float(r2_of(radius)) == 25 * nc.LATTICE_RIM_STEP ** 2 and (kp == np.arange(0, len(xyz), 5)).all()
    at_rim = d2_f32(xyz[pairs[:, 0]], xyz[pairs[:, 1]]) == r2_of(radius)
    assert (at_rim == (d2i == 25)).all() and at_rim.sum() >= 1000
    # ordered pairs one float step of d2 below the rim (24 = 16 + 4 + 4 lattice steps squared): accepted
    assert (ref.d2.astype(np.float64) == 24 * nc.LATTICE_RIM_STEP ** 2).sum() >= 2000
    assert not (ref.d2 >= r2_of(radius)).any()


@pytest.mark.parametrize("name", fc.CLOUD_CASES)
def test_nonfirm_rows_stay_under_the_cap(name):
    ref = fc.case_reference(name)
    share = fc.nonfirm_share(ref)
    print(name, "computed rows", int(ref.union.sum()), "feature pairs", len(ref.pair_firm), "non-firm pairs",
          int((~ref.pair_firm).sum()), "non-firm rows %.2f %%" % (100 * share))
    assert ref.union.sum() >= 100
    assert share <= fc.NONFIRM_CAP


@pytest.mark.parametrize("name", fc.CASES)
def test_float_model_gives_the_truth_bins_on_firm_pairs(name):
    xyz, nrm, _kp, _radius = fc.case(name)
    ref = fc.case_reference(name)
    pts, nr = xyz[ref.fin_idx], nrm[ref.fin_idx]
    valid, bins = fc.pair_model(pts[ref.pair_I], nr[ref.pair_I], pts[ref.pair_J], nr[ref.pair_J])
    firm = ref.pair_firm
    differ = (valid != ref.pair_valid) | (bins != ref.pair_bins).any(1)
    print(name, "pairs", len(firm), "model differs on", int(differ.sum()), "of them firm", int((differ & firm).sum()))
    assert not (differ & firm).any()


def test_histogram_reference_properties():
    """the fp64 weighting: each feature's bins sum to 100 or are all 0; lone keypoints are zero rows"""
    for name in ("part_kp", "dups", "n1", "n2"):
        h, m, _firm, lone = fc.case_histograms(name)
        ok = ~np.isnan(h[:, 0])
        for f in range(3):
            s = h[ok, 11 * f:11 * f + 11].sum(1)
            assert (np.isclose(s, 100.0, rtol=0, atol=1e-9) | (s == 0)).all()
        assert not h[lone].any() and (m[ok] >= 1).all()
    assert fc.case_histograms("n1")[3].all() and not fc.case_histograms("n2")[3].any()


def test_fpfh_adapter_compiles_against_standins():
    """adapter/InitialAlignment_mi355x.cpp compiles as the catkin package would compile it, against
    the stand-in headers of tests/adapter_standins_ia, and links to libmgicp.so through product symbols only."""
    from leica_point_cloud_processing_amd import _lib

    r = subprocess.run(["make", "-s", "-C", ROOT, "fpfh-replay"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_fpfh")
    assert os.path.exists(exe)
    nm = subprocess.run(["nm", "-C", exe], capture_output=True, text=True).stdout
    assert "InitialAlignment::obtainFeatures" in nm
    needed = {line.split()[-1] for line in subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout.splitlines()
              if line.split() and line.split()[-1].startswith("mgicp_")}
    assert "mgicp_fpfh_features" in needed and "mgicp_cloud_resolution" in needed
    assert needed <= set(_lib.header_symbols(_lib.HEADER_PATH)), sorted(needed)


def test_python_binding_matches_header():
    """mgicp_fpfh_info: the ctypes mirror has the header's fields in the header's order, all double."""
    import ctypes
    import re

    from leica_point_cloud_processing_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*mgicp_fpfh_info;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"\b(double|int)\s+([\w\s,]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert [(n, {"double": ctypes.c_double, "int": ctypes.c_int}[t]) for n, t in fields] == list(_lib.MgicpFpfhInfo._fields_)
    assert len(fields) == 9 and ctypes.sizeof(_lib.MgicpFpfhInfo) == 72
    assert "mgicp_fpfh_features" in _lib._SIGNATURES and len(_lib._SIGNATURES["mgicp_fpfh_features"][1]) == 14
    assert "mgicp_fpfh_features" in _lib.header_symbols(_lib.HEADER_PATH)


def test_obtainFeatures_refuses_without_an_engine():
    """the -1 of mismatched normals or of no keypoint comes before any device work (PCL's initCompute)"""
    from leica_point_cloud_processing_amd.initial_alignment import obtainFeatures

    status, feats = obtainFeatures(np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float32), [0, 1])
    assert status == -1 and feats.shape == (0, 33)
    status, feats = obtainFeatures(np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), [])
    assert status == -1 and feats.shape == (0, 33)
