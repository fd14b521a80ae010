"""The cases of tests/normal_cluster_cases.py, checked on the CPU: each case's premise holds, and every decision
of the reference is firm -- no dot within 4 float32 steps of c_min (except in the cases built for the
threshold) and no candidate pair's d2 within 4 steps of float32(tol^2) (except the pairs the 1 mm planes place
at the tolerance itself).  No case is skipped.  Also: the header and the ctypes table name the two calls."""
import math
import os

import numpy as np
import pytest

import normal_cluster_cases as nc

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_min_of_20_degrees_is_the_headers():
    cm = nc.c_min(nc.EPS)
    assert cm == F32(0.9396927) and math.acos(float(cm)) < nc.EPS
    below = np.nextafter(cm, F32(-2.0))
    assert below == F32(0.9396926) and not math.acos(float(below)) < nc.EPS
    assert nc.c_min(0.0) == F32(np.inf) and nc.c_min(4.0) == F32(-1.0)
    assert nc.c_min(math.pi) == np.nextafter(F32(-1.0), F32(2.0))  # acos(-1) = pi is not below pi


@pytest.mark.parametrize("name", nc.CASES)
def test_every_reference_decision_is_firm(name):
    c, ref = nc.case(name), nc.case_reference(name)
    if not c.threshold_case:
        assert ref.dot_steps > 4, ref.dot_steps
    if not c.placed_pairs:
        assert ref.d2_steps > 4, ref.d2_steps
        assert not ref.near_pairs


def test_the_planes_place_pairs_at_the_tolerance_and_nowhere_near_it():
    """the pairs within 4 steps of float32(tol^2) are exactly the lattice offsets whose length is 50 mm"""
    c, ref = nc.case("plane"), nc.case_reference("plane")
    assert ref.near_pairs
    ij = np.rint(c.xyz[:, :2].astype(np.float64) / 0.001).astype(int)
    for p, j in ref.near_pairs:
        d = np.abs(ij[p] - ij[j])
        assert d[0] ** 2 + d[1] ** 2 == 2500, (p, j, d)
    # re-derived in float in the far frame: the x coordinates are multiples of 2^-11 m there, so of the
    # lattice offsets only (0, +-50 mm) -- equal x, 50 rows apart in y -- can still sit on the tolerance
    far, xyz = nc.case_reference("far_plane"), nc.case("far_plane").xyz
    assert far.near_pairs
    for p, j in far.near_pairs:
        assert xyz[p, 0] == xyz[j, 0] and abs(p % 60 - j % 60) == 50 and xyz[p, 2] == xyz[j, 2], (p, j)


def test_the_seed_rule_is_not_the_chain_rule():
    end, mid = nc.case_reference("line_end"), nc.case_reference("line_middle")
    # index 0 at one end: positions 0 .. 4 are within 20 degrees of position 0 (19 < 20 < 23.75), then fives
    assert [len(m) for m in end.rounds] == [5] * 8 and end.rounds[0].tolist() == [0, 1, 2, 3, 4]
    # index 0 in the middle (position 20): a symmetric first cluster of nine
    pos = nc.case("line_middle").pos
    assert sorted(pos[mid.rounds[0]].tolist()) == list(range(16, 25))
    assert [len(m) for m in mid.rounds] != [len(m) for m in end.rounds]
    assert max(len(m) for m in mid.rounds) < 40  # the chain rule would take all 40


def test_consumption_blocks_paths():
    c, ref = nc.case("bridge"), nc.case_reference("bridge")
    assert [m.tolist() for m in ref.rounds] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    # without the bridge's consumption seed 3 reaches the other side: the same records with record 0 moved away
    xyz = c.xyz.copy()
    xyz[0] = (10, 10, 10)
    free = nc.reference(xyz, c.normals)
    assert [1, 2, 3, 4, 5, 6, 7, 8] in [m.tolist() for m in free.rounds] or free.rounds[1].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    # the two sides are more than tol apart
    assert nc.d2_float(c.xyz[5], c.xyz[6]) > F32(nc.TOL * nc.TOL)


def test_a_dropped_cluster_still_consumes():
    ref = nc.case_reference("dropped")
    assert ref.rounds[0].tolist() == [0, 5] and ref.labels[5] == -1 and ref.labels[0] == -1
    assert [m.tolist() for m in ref.clusters] == [[1, 2, 3, 4, 6, 7, 8, 9]]
    c = nc.case("dropped")
    assert nc.dot_float(c.normals[1], c.normals[5]) >= nc.c_min(nc.EPS)  # 5 is compatible with seed 1


def test_a_self_dot_above_one_gives_singletons():
    above, unit = nc.case("patch_above_one"), nc.case("patch_unit")
    assert nc.dot_float(above.normals[0], above.normals[0]) == np.nextafter(F32(1.0), F32(2.0))
    assert nc.dot_float(unit.normals[0], unit.normals[0]) <= F32(1.0)
    assert nc.case_reference("patch_above_one").n_rounds == 100
    assert [len(m) for m in nc.case_reference("patch_unit").rounds] == [100]


def test_the_threshold_case_sits_on_the_threshold():
    c = nc.case("threshold_20deg")
    cm = nc.c_min(nc.EPS)
    d = nc.dot_float(c.normals[0], c.normals)
    assert d.tolist() == [1.0, float(cm), float(np.nextafter(cm, F32(-2.0))), 1.0, -1.0]
    assert nc.case_reference("threshold_20deg").rounds[0].tolist() == [0, 1, 3]
    assert nc.case_reference("threshold_eps_0").n_rounds == 5
    assert nc.case_reference("threshold_eps_4").rounds[0].tolist() == [0, 1, 2, 3, 4]


def test_odd_records():
    ref = nc.case_reference("odd_records")
    assert [m.tolist() for m in ref.rounds] == [[0], [1], [3, 4, 5]]
    assert ref.labels.tolist() == [0, 1, -1, 2, 2, 2]


def test_long_rounds_and_many_rounds():
    assert [len(m) for m in nc.case_reference("long_line").rounds] == [300]
    assert [len(m) for m in nc.case_reference("plane").rounds] == [3600]
    assert [len(m) for m in nc.case_reference("far_plane").rounds] == [3600]
    assert [len(m) for m in nc.case_reference("blob").rounds] == [4200]
    assert len(nc.case("blob").xyz) - 1 > 4096  # the LDS frontier's entries (the debug header's limit range) and 4096 in nc.case("blob").limits
    lat = nc.case_reference("lattice")
    assert lat.n_rounds == 4096 and all(len(m) == 1 for m in lat.rounds)
    cos = nc.CORNERS.astype(np.float64) @ nc.CORNERS.astype(np.float64).T
    assert np.all(cos[~np.eye(8, dtype=bool)] < math.cos(math.radians(45)))
    for c in (nc.case("long_line"), nc.case("plane"), nc.case("far_plane")):
        size = len(c.xyz)
        assert c.limits == (0, 1, size - 1, size, size + 1)


def test_the_tree_restatement_counts_the_first_member_twice():
    normals, clusters = nc.dominant_case()
    assert tuple(len(m) for m in clusters) == nc.DOMINANT_SIZES
    twice, sums = nc.dominant_reference(normals, clusters)
    once, _ = nc.dominant_reference(normals, clusters, first_twice=False)
    assert np.all(np.any(twice[1:6] != once[1:6], axis=1))  # (a single member's normal is itself either way)
    # the tree is a sum: within the standard bound of the correctly rounded one
    for c, m in enumerate(clusters):
        e = np.concatenate([m[:1], m])
        exact = np.array([math.fsum(normals[e, r].astype(np.float64)) for r in range(3)])
        assert np.all(np.abs(sums[c] - exact) <= len(e) * 2.0 ** -52 * len(e))
    assert nc.tree_sum([1.0, 2.0, 4.0]) == (1.0 + 4.0) + 2.0  # the header's n = 3 example


def test_the_header_and_the_ctypes_table_name_both_calls():
    from leica_point_cloud_processing_amd import _lib

    names = {"mgicp_normal_clusters", "mgicp_dominant_normals"}
    assert names <= set(_lib.header_symbols(os.path.join(ROOT, "include", "mi355x_gicp.h")))
    assert names <= set(_lib._SIGNATURES)
    with open(os.path.join(ROOT, "include", "mi355x_gicp.h")) as f:
        text = f.read()
    assert "unpinned against PCL binaries" in text and "mgicp_normal_cluster_info" in text
