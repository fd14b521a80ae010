"""CPU checks of the radius-normal cases (tests/normals_cases.py): every cloud is what it claims to be,
few records are excluded from the direction and sign comparisons, and the bounds the GPU tests assert
hold for a NumPy model of the arithmetic mgicp_estimate_normals is specified to use -- with room to
PCL's float arithmetic on the other side.  Also: the adapter's Utils::getNormals compiles."""
import os
import subprocess

import numpy as np
import pytest

import normals_cases as nc
from conftest import ROOT


@pytest.mark.parametrize("name", nc.DIRECTION_CASES)
def test_few_records_are_excluded(name):
    """At most 1 % of a case's non-NaN records have a relative eigen-gap below GAP_MIN (no stable normal
    in any arithmetic) and at most 1 % a view direction within COS_MIN of the tangent plane."""
    xyz, _radius = nc.case(name)
    ref = nc.case_reference(name)
    has = ref.has
    assert has.sum() > 0
    low_gap = has & ~(ref.gap_rel >= nc.GAP_MIN)
    print(name, "records", len(xyz), "with a normal", int(has.sum()), "gap below", nc.GAP_MIN, int(low_gap.sum()))
    assert low_gap.sum() <= 0.01 * has.sum()
    extra = nc.viewpoints()
    for vp in ((0.0, 0.0, 0.0),) + ((extra[name],) if name in extra else ()):
        _sign, cos = nc.orientation(xyz, ref, vp)
        grazing = has & ~(cos >= nc.COS_MIN)
        print(name, "viewpoint", vp, "grazing", int(grazing.sum()))
        if name == "far_sheet_origin" and vp == (0.0, 0.0, 0.0):
            # the control's sheet x = 0.3 y - 0.2 z passes through the default viewpoint: every view direction
            # lies in the plane up to the sheet's noise.  The cap holds at the case's own viewpoint (below);
            # the sign test at the origin compares whatever COS_MIN leaves
            plane = np.asarray(nc.FAR_SHEET_PLANE) / np.linalg.norm(nc.FAR_SHEET_PLANE)
            assert np.abs(xyz.astype(np.float64) @ plane).max() < 1e-3 and name in extra
            continue
        assert grazing.sum() <= 0.01 * has.sum()


@pytest.mark.parametrize("name", nc.DIRECTION_CASES)
def test_model_meets_the_bounds(name):
    """The specified arithmetic (fp64 raw moments of the differences) in NumPy: its normals are within
    DIR_BOUND / gap_rel of the truth and its worst angle is below the MEDIAN angle of PCL's float
    arithmetic on the same records; its curvature is within CURV_BOUND less the float rounding of the
    output (2^-26 for a value of at most 1/3)."""
    ref = nc.case_reference(name)
    sel = ref.has & (ref.gap_rel >= nc.GAP_MIN)
    worst = float(ref.model_angle[sel].max())
    pcl_median = float(np.median(ref.pcl_angle[sel]))
    print(name, "model worst angle", worst, "pcl median", pcl_median, "pcl max", float(ref.pcl_angle[sel].max()))
    assert (ref.model_angle[sel] <= nc.DIR_BOUND / ref.gap_rel[sel] - 2.0 ** -24 * np.sqrt(3.0)).all()
    assert worst <= pcl_median
    assert np.abs(ref.model_curvature[ref.has] - ref.curvature[ref.has]).max() <= nc.CURV_BOUND - 2.0 ** -26


def test_case_shapes():
    """Each cloud reaches the part of the kernel it is there for."""
    for name in nc.DIRECTION_CASES:
        assert len(nc.case(name)[0]) <= 6000, name
    cube, part, small = nc.case_reference("cube"), nc.case_reference("part"), nc.case_reference("part_small")
    xyz, _ = nc.case("cube")
    assert cube.has.all() and cube.count.min() >= 200 and cube.count.max() <= 500
    assert (xyz.min(0) < 0).all() and (xyz.max(0) > 0).all()  # the default viewpoint lies inside
    assert part.has.all() and 30 <= part.count.min() and part.count.max() <= 320
    assert 0 < (~small.has).sum() < 0.1 * len(small.has) and small.count.max() <= 40
    # clump: one cell with more points than a block has lanes, a neighbourhood past one staging chunk
    xyz, radius = nc.case("clump")
    h, most, _dims = nc.grid_facts(xyz, radius)
    assert h == radius and most > nc.BLOCK_LANES and most > nc.STAGE_POINTS
    assert nc.case_reference("clump").count.max() > nc.STAGE_POINTS
    # huge radius: one cell, every point neighbours every point
    xyz, radius = nc.case("huge_radius")
    h, most, dims = nc.grid_facts(xyz, radius)
    assert dims == [1, 1, 1] and most == len(xyz) == 777 and len(xyz) % 64
    assert (nc.case_reference("huge_radius").count == 777).all()
    assert radius > np.linalg.norm(xyz.max(0) - xyz.min(0))
    # tiny radius: the cell edge is grown past the radius; most records have no normal
    xyz, radius = nc.case("tiny_radius")
    h, _most, dims = nc.grid_facts(xyz, radius)
    ref = nc.case_reference("tiny_radius")
    assert h > 5 * radius and max(dims) == 1 << 20
    assert ref.has.sum() == 30 and (~ref.has).sum() == 600
    # non-finite records: present, and without a normal
    xyz, _ = nc.case("nonfinite")
    bad = ~np.isfinite(xyz).all(1)
    ref = nc.case_reference("nonfinite")
    assert bad.sum() == 50 and np.isnan(xyz).any() and np.isposinf(xyz).any() and np.isneginf(xyz).any()
    assert not ref.has[bad].any() and (ref.count[bad] == 0).all() and ref.has[~bad].sum() > 2000


def test_far_sheet_regimes():
    """far_sheet: the grid's slop exceeds the radius, so a single query's cell box (cell_box; a group's box in
    normals_tile_kernel is at least as large) has more than 64 rows of cells and more points than one staged
    chunk for at least a third of the records -- on both sides of the origin -- while the control, the same
    draws at X0 = 0, has no box above 4 x 4 rows.  Conditions on the inputs, from the float32 restatement of
    the cell function; nothing here measures the engine."""
    ctrl, radius = nc.case("far_sheet_origin")
    rows0, pts0, rel0 = nc.box_facts(ctrl, radius)
    h, _most, dims = nc.grid_facts(ctrl, radius)
    print("far_sheet_origin rx / h", rel0, "rows max", int(rows0.max()), "points max", int(pts0.max()), "dims", dims)
    assert h == radius and rel0 < 1.001 and rows0.max() <= 16 and pts0.max() <= nc.STAGE_POINTS
    for name in ("far_sheet", "far_sheet_neg"):
        xyz, r = nc.case(name)
        x0 = nc.FAR_SHEET_X0[name]
        assert r == radius and len(xyz) == 6000 and len(np.unique(xyz, axis=0)) == 6000
        # the same draws in another frame: y and z bit for bit, x within half a float step of X0 + the control's
        assert (xyz[:, 1:] == ctrl[:, 1:]).all()
        assert np.abs((xyz[:, 0].astype(np.float64) - x0) - ctrl[:, 0]).max() <= 2.0 ** -12 + 2.0 ** -30
        assert np.sign(xyz[:, 0]).min() == np.sign(xyz[:, 0]).max() == np.sign(x0)
        rows, pts, rel = nc.box_facts(xyz, r)
        h, _most, dims = nc.grid_facts(xyz, r)
        print(name, "rx / h", rel, "rows: share above 64", float((rows > 64).mean()), "max", int(rows.max()),
              "points: share above", nc.STAGE_POINTS, float((pts > nc.STAGE_POINTS).mean()), "max", int(pts.max()),
              "dims", dims)
        assert h == r and rel > 4.0                                 # the slop alone is three cell edges
        assert (rows > 64).sum() * 3 >= len(xyz)                    # fpfh_walk's second turn of 64 rows
        assert (pts > nc.STAGE_POINTS).sum() * 3 >= len(xyz)        # more than one staged chunk per group
        ref = nc.case_reference(name)
        assert ref.has.all() and (ref.gap_rel >= nc.GAP_MIN).all()


def test_far_part_is_the_part_shifted():
    """far_part: the first 3000 records of the part's scan plus a site offset, added in float32; the offsets
    are those of the geometry-edge tests; the non-default viewpoint moves with the cloud"""
    from geometry_edges_cases import OFFSETS

    scan, _res = nc._part_scan()
    for name, site in nc.FAR_PART_OFFSET.items():
        xyz, radius = nc.case(name)
        off = np.asarray(OFFSETS[site], np.float32)
        assert np.abs(off).max() >= 300 and (xyz == scan[:3000] + off).all() and xyz.dtype == np.float32
        assert radius == 10.0 * nc.resolution(scan[:3000])
        assert nc.viewpoints()[name] == tuple((np.asarray(nc.VIEWPOINT, np.float32) + off).tolist())
        ref = nc.case_reference(name)
        assert ref.has.all() and (ref.gap_rel >= nc.GAP_MIN).all()
        assert np.linalg.norm(xyz.astype(np.float64), axis=1).min() > 300  # the default viewpoint is far away


def test_lattice_rim_pairs_are_exact():
    """lattice_rim: every float d2 is the integer lattice d2 times 2^-22 exactly, float(radius^2) is 25 of
    them, and thousands of pairs sit at d2 == r2 (rejected) and one float step below (24: accepted) -- the
    sets are decided by the strictness of the test alone.  The reference's counts are the integer counts."""
    from scipy.spatial import cKDTree

    xyz, radius = nc.case("lattice_rim")
    ij = nc.lattice_rim_ij()
    step = nc.LATTICE_RIM_STEP
    assert len(np.unique(ij, axis=0)) == len(ij) == len(xyz) >= 5000
    assert (xyz.astype(np.float64) == np.asarray(nc.LATTICE_RIM_OFF) + ij * step).all()
    mag = np.abs(xyz)
    assert ((mag >= 4096) & (mag < 8192)).all()  # one binade: the float step is 2^-11 for every coordinate
    assert (np.abs(np.nextafter(xyz, np.float32(np.inf)) - xyz) == np.float32(step)).all()
    r2 = nc.r2_of(radius)
    assert float(r2) == 25 * step * step
    pairs = cKDTree(ij).query_pairs(np.sqrt(40.5), output_type="ndarray")  # every pair with an integer d2 <= 40
    a, b = pairs[:, 0], pairs[:, 1]
    d2i = ((ij[a] - ij[b]) ** 2).sum(1)
    assert (nc.d2_f32(xyz[a], xyz[b]).astype(np.float64) == d2i * (step * step)).all()
    assert (nc.d2_f32(xyz[b], xyz[a]).astype(np.float64) == d2i * (step * step)).all()
    at_rim, below = int((d2i == 25).sum()), int((d2i == 24).sum())
    rim_records = int((np.bincount(pairs[d2i == 25].ravel(), minlength=len(ij)) > 0).sum())
    print("lattice_rim records", len(xyz), "pairs at d2 == r2", at_rim, "one step below", below, "accepted",
          int((d2i < 25).sum()), "records with a pair at the rim", rim_records)
    assert at_rim >= 1000 and below >= 1000
    assert not ((d2i > 24) & (d2i < 25)).any()  # integers: nothing between the last accepted and the rim
    ref = nc.case_reference("lattice_rim")
    np.testing.assert_array_equal(ref.count, 1 + np.bincount(pairs[d2i < 25].ravel(), minlength=len(ij)))
    # slop over radius: the box is three cells wide on either side (the grid: cells of one radius)
    _rows, _pts, rel = nc.box_facts(xyz, radius)
    h, _most, dims = nc.grid_facts(xyz, radius)
    print("lattice_rim rx / h", rel, "dims", dims)
    assert h == radius and 2.5 < rel < 3.5


def test_degenerate_and_edge_clouds():
    xyz, radius, rows = nc.degenerate()
    ref = nc.reference(xyz, radius)
    assert ref.has[rows].all()
    # no plane: the two smallest eigenvalues of the centred covariance vanish against the largest, or all do
    _fin, I, J = nc.neighbour_pairs(xyz, radius)
    for i in rows:
        nb = xyz[J[I == i]].astype(np.float64)
        w = np.linalg.eigvalsh(np.cov(nb.T, bias=True))
        assert w[1] <= 1e-9 * max(w[2], 1e-30) or w[2] == 0, (i, w)
    edge = nc.edge_clouds()
    assert nc.r2_of(edge["radius_zero"][1]) == 0
    r2 = nc.r2_of(edge["denormal_r2"][1])
    assert 0 < r2 < np.float32(1.17549435e-38)
    cnt = nc.reference(*edge["denormal_r2"]).count
    assert sorted(np.unique(cnt)) == [1, 2, 3] and (cnt[:3] == 3).all() and (cnt[3:6] == 2).all()
    assert [len(edge[k][0]) for k in ("n0", "n1", "n2_near", "n2_far")] == [0, 1, 2, 2]
    assert list(nc.reference(*edge["n2_near"]).count) == [2, 2] and list(nc.reference(*edge["n2_far"]).count) == [1, 1]


def test_normals_adapter_compiles_against_standins():
    """adapter/Utils_mi355x.cpp passes g++ -std=c++14 -Wall -Wextra -Werror against the stand-ins of
    tests/adapter_standins_normals and links to libmgicp.so through product symbols only."""
    from leica_point_cloud_processing_amd import _lib

    r = subprocess.run(["make", "-s", "-C", ROOT, "normals-replay"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(ROOT, "adapter", "build", "replay_test_normals")
    assert os.path.exists(exe)
    nm = subprocess.run(["nm", "-C", exe], capture_output=True, text=True).stdout
    assert "Utils::getNormals" in nm
    needed = {line.split()[-1] for line in subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout.splitlines()
              if line.split() and line.split()[-1].startswith("mgicp_")}
    assert "mgicp_estimate_normals" in needed
    assert needed <= set(_lib.header_symbols(_lib.HEADER_PATH)), sorted(needed)


def test_python_binding_matches_header():
    """mgicp_normals_info: the ctypes mirror has the header's fields in the header's order, all double."""
    import ctypes
    import re

    from leica_point_cloud_processing_amd import _lib

    text = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*mgicp_normals_info;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(double|int)\s+(\w+)\s*;", body)
    assert [(n, {"double": ctypes.c_double, "int": ctypes.c_int}[t]) for t, n in fields] == list(_lib.MgicpNormalsInfo._fields_)
    assert "mgicp_estimate_normals" in _lib._SIGNATURES
    assert "mgicp_estimate_normals" in _lib.header_symbols(_lib.HEADER_PATH)
