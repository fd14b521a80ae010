"""CPU tests of the boundary-estimation cases (tests/boundary_cases.py): every cloud is what it claims to
be, the regimes of the kernels are reached, and the float32 model of the specified arithmetic stays within
the bound the GPU tests hold the engine to -- so that bound is about the arithmetic, not about the engine.
Also: the adapter compiles against its stand-ins, and the ctypes mirror matches the header."""
import os
import subprocess

import numpy as np
import pytest

import boundary_cases as bc
import normals_cases as nc
from conftest import ROOT

# the cases whose geometry allows interior and boundary records; at k = 7 six neighbours cannot close
# every gap below 60 degrees, `few` is ten points and `one_angle`'s far sheet is sparse: all boundary
MIXED_CASES = tuple(c for c in bc.CASES if c not in ("k7", "few", "one_angle"))


@pytest.mark.parametrize("name", bc.CASES)
def test_reference_shapes_and_rules(name):
    xyz, nrm, k = bc.case(name)
    ref = bc.case_reference(name)
    n = len(xyz)
    assert xyz.dtype == np.float32 and nrm.dtype == np.float32 and nrm.shape == (n, 3)
    assert ref.nn.shape == (n, k) and ref.nn.dtype == np.int32
    fin = np.isfinite(xyz).all(1)
    assert ref.n_finite == fin.sum()
    assert (ref.nn[~fin] == -1).all()
    np.testing.assert_array_equal(ref.size, (ref.nn >= 0).sum(1))
    np.testing.assert_array_equal(ref.size[fin], min(k, ref.n_finite))
    # a row starts with the record itself or a duplicate of it with a lower index; the padding is at the end
    first = ref.nn[fin, 0]
    assert (first <= np.flatnonzero(fin)).all() and (xyz[first] == xyz[fin]).all()
    assert ((ref.nn >= 0)[:, :-1] >= (ref.nn >= 0)[:, 1:]).all()
    # members are finite records, each once
    rows = ref.nn[fin]
    assert fin[rows[rows >= 0]].all()
    srt = np.sort(rows, axis=1)
    assert ((srt[:, 1:] != srt[:, :-1]) | (srt[:, 1:] < 0)).all()
    # not decided: exactly the four rules
    has_normal = np.isfinite(nrm).all(1)
    delta_all_zero = np.array([(xyz[r[r >= 0]] == xyz[i]).all() for i, r in enumerate(ref.nn)]) if n else np.zeros(0, bool)
    np.testing.assert_array_equal(ref.decided, fin & has_normal & (ref.size >= 3) & ~delta_all_zero)
    assert np.isnan(ref.truth[~ref.decided]).all() and np.isnan(ref.model[~ref.decided]).all()
    assert np.isfinite(ref.truth[ref.decided]).all() and np.isfinite(ref.model[ref.decided]).all()


@pytest.mark.parametrize("name", bc.CASES)
def test_ties_at_the_kth_place(name):
    """float d2 ties across the k-th place exist where the case is built for them and nowhere else, so
    every other case's sets do not depend on the tie rule"""
    ref = bc.case_reference(name)
    print(name, "records with a tie at the k-th place", int(ref.tie.sum()))
    if name in bc.TIE_CASES:
        assert ref.tie.sum() >= 50
    else:
        assert ref.tie.sum() == 0


def test_regime_certificates():
    # pile: more than LOG_CAP records within the k-th distance -- every entry with d2 <= the final k-th
    # must be in the log at the end, so these queries overflow it and take the hand-off launch
    ref = bc.case_reference("pile")
    over = ref.n_le > bc.LOG_CAP
    print("pile: queries certain to overflow the log", int(over.sum()), "decided among them", int((over & ref.decided).sum()))
    assert (over & ref.decided).sum() >= 20
    # ... and in every other case no query comes near the capacity with its final set alone
    for name in bc.CASES:
        if name != "pile":
            assert bc.case_reference(name).n_le.max() <= bc.LOG_CAP - 8, name
    # lattice: more ties than places left -- the lowest-index rule decides the set
    ref = bc.case_reference("lattice")
    assert (ref.tie & (ref.n_le > 30)).sum() >= 50
    # lattice_rim: the same in a frame of 2^-11 steps, where most records tie
    ref = bc.case_reference("lattice_rim")
    assert (ref.tie & (ref.n_le > 30)).sum() >= 50
    # clump: k = 32 fills the list without sentinels; the crowded disc puts 1500 points in a 2 cm spot
    xyz, _nrm, k = bc.case("clump")
    assert k == 32 and len(xyz) == 3100
    # huge_radius: 777 points, no multiple of the 64 queries of a block
    assert len(bc.case("huge_radius")[0]) == 777 and 777 % 64
    # outliers: the 40 far records have no normal, and their sets are the decided records' business only
    xyz, nrm, _k = bc.case("outliers")
    far = np.abs(xyz).max(1) > 20
    assert far.sum() == 40 and np.isnan(nrm[far]).all() and np.isfinite(nrm[~far]).all()
    assert not bc.case_reference("outliers").decided[far].any()


def _kth_distance(name):
    xyz, _nrm, k = bc.case(name)
    ref = bc.case_reference(name)
    assert (ref.size == k).all()
    return np.sqrt(bc.d2_f32(xyz, xyz[ref.nn[:, k - 1]]).astype(np.float64))


def test_far_frame_certificates():
    """far_sheet: the slop of any grid over the cloud (8 float steps of the largest coordinate, whatever the
    cell edge) exceeds every record's k-th neighbour distance, so ring_search's bound L 0.99999 - slop proves
    nothing until the unvisited cells are a slop farther than the k-th neighbour -- neighbours near, bounds
    weak -- where the control at X0 = 0 has a slop below a thousandth of that distance.  How many queries then
    reach the ring cap depends on the auto-sized cell edge, which the CPU side does not restate: the GPU tests
    assert parity whichever path a query takes.  far_part: the same sets as a reference of the shifted cloud,
    no ties; truth normals everywhere."""
    for name in nc.FAR_SHEET_X0:
        xyz, nrm, k = bc.case(name)
        slop = 8.0 * float(np.abs(xyz).max()) * 2.0 ** -23
        kth = _kth_distance(name)
        print(name, "slop", slop, "k-th neighbour distance", float(kth.min()), "-", float(kth.max()))
        assert k == bc.K_DEFAULT and np.isfinite(nrm).all() and bc.case_reference(name).decided.all()
        if name == "far_sheet_origin":
            assert slop < 1e-3 * kth.min()
        else:
            assert slop > kth.max() and slop > 3 * nc.FAR_SHEET_RADIUS
        assert (np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1) < 1e-6).all()
    for name in nc.FAR_PART_OFFSET:
        xyz, nrm, k = bc.case(name)
        assert k == bc.K_DEFAULT and len(xyz) == 3000 and np.isfinite(nrm).all()
        assert (nrm == bc.truth_normals(xyz, nc.case(name)[1])).all()
        assert bc.case_reference(name).decided.all()
    xyz, nrm, k = bc.case("lattice_rim")
    assert k == bc.K_DEFAULT and (xyz == nc.lattice_rim()[0]).all() and np.isfinite(nrm).all()
    ref = bc.case_reference("lattice_rim")
    assert ref.tie.sum() * 2 >= len(xyz)  # ties are the norm: the (d2, original index) rule decides most sets


def test_small_case_facts():
    xyz, _nrm, k = bc.case("few")
    ref = bc.case_reference("few")
    fin = np.isfinite(xyz).all(1)
    assert fin.sum() == 10 and k == 30 and (ref.size[fin] == 10).all() and ref.decided[fin].all()
    # dups: every point three times; two members of every set have delta = 0
    xyz, _nrm, k = bc.case("dups")
    ref = bc.case_reference("dups")
    _u, cnt = np.unique(xyz, axis=0, return_counts=True)
    assert (cnt == 3).all() and ref.decided.all()
    assert all((xyz[r] == xyz[i]).all(1).sum() == 3 for i, r in enumerate(ref.nn))
    # one_angle: records 0-2 are one point, their 4-sets hold record 3 as the only other member
    xyz, _nrm, k = bc.case("one_angle")
    ref = bc.case_reference("one_angle")
    assert k == 4 and (xyz[:3] == xyz[0]).all()
    for i in range(3):
        assert sorted(ref.nn[i]) == [0, 1, 2, 3]
        assert abs(ref.truth[i] - 2 * np.pi) < 1e-12 and abs(float(ref.model[i]) - 2 * np.pi) <= bc.bound(1.0)


@pytest.mark.parametrize("name", bc.CASES)
def test_model_within_bound_of_truth(name):
    ref = bc.case_reference(name)
    _xyz, nrm, _k = bc.case(name)
    gap_ok, flag_ok = bc.comparable(ref)
    err = np.abs(ref.model.astype(np.float64) - ref.truth)
    worst = float((err[gap_ok] / bc.bound(ref.sens[gap_ok])).max())
    thr = np.float32(bc.THRESHOLD)
    flips = int(((ref.model > thr) != (ref.truth > np.float64(thr)))[flag_ok].sum())
    with_normal = int((np.isfinite(nrm).all(1) & (ref.size > 0)).sum())
    left_out = int((ref.decided & ~flag_ok).sum())
    print(name, "compared", int(gap_ok.sum()), "worst error / bound", worst, "largest sens", float(ref.sens[ref.decided].max()),
          "left out", left_out, "of", with_normal)
    assert (err[gap_ok] <= bc.bound(ref.sens[gap_ok])).all()
    assert flips == 0
    # the cap: a condition on the reference alone
    assert left_out <= bc.LEFT_OUT_MAX * with_normal


@pytest.mark.parametrize("name", MIXED_CASES)
def test_neither_none_nor_all_are_boundary_points(name):
    ref = bc.case_reference(name)
    b = ref.truth[ref.decided] > np.float64(np.float32(bc.THRESHOLD))
    print(name, "boundary points", int(b.sum()), "of", len(b))
    assert 0 < b.sum() < len(b)


def test_boundary_adapter_compiles_against_standins():
    """adapter/InitialAlignment_mi355x.cpp passes g++ -std=c++14 -Wall -Wextra -Werror against the stand-ins
    of tests/adapter_standins_ia and links to libmgicp.so through product symbols only."""
    from leica_point_cloud_processing_amd import _lib

    r = subprocess.run(["make", "-s", "-C", ROOT, "boundary-replay"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_boundary")
    assert os.path.exists(exe)
    nm = subprocess.run(["nm", "-C", exe], capture_output=True, text=True).stdout
    assert "InitialAlignment::obtainBoundaryKeypoints" in nm
    needed = {line.split()[-1] for line in subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout.splitlines()
              if line.split() and line.split()[-1].startswith("mgicp_")}
    assert "mgicp_boundary_points" in needed
    assert needed <= set(_lib.header_symbols(_lib.HEADER_PATH)), sorted(needed)


def test_python_binding_matches_header():
    """mgicp_boundary_info: the ctypes mirror has the header's fields in the header's order, all double."""
    import ctypes
    import re

    from leica_point_cloud_processing_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*mgicp_boundary_info;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(double|int)\s+(\w+)\s*;", body)
    assert [(n, {"double": ctypes.c_double, "int": ctypes.c_int}[t]) for t, n in fields] == list(_lib.MgicpBoundaryInfo._fields_)
    assert len(fields) == 7
    assert "mgicp_boundary_points" in _lib._SIGNATURES
    assert "mgicp_boundary_points" in _lib.header_symbols(_lib.HEADER_PATH)


def test_obtainBoundaryKeypoints_refuses_mismatched_normals_without_an_engine():
    """the -1 of a size mismatch comes before any device work (PCL's initCompute)"""
    from leica_point_cloud_processing_amd.initial_alignment import obtainBoundaryKeypoints

    status, kp, nkp = obtainBoundaryKeypoints(np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float32))
    assert status == -1 and len(kp) == 0 and len(nkp) == 0
