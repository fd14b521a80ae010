"""mgicp_euclidean_clusters and mgicp_voxel_grid against their references where the device code's float
margins are tight (clouds: tests/cluster_edges_cases.py, certified by tests/test_cluster_edges_inputs.py).

The bar is exact equality throughout: clusters, their order, members, labels, offsets and n_components
against `ref_clusters` (the fp32 FLANN predicate in numpy); voxel xyz and rgba bit for bit against
oracle.ref.voxel_grid.
"""
import numpy as np
import pytest

import cluster_edges_cases as cc
from geometry_edges_cases import OFFSETS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    e = GICPEngine()
    yield e
    e.close()


def _assert_same(got, ref):
    """exact equality of the whole result; the clusters are compared as one concatenation (32 768 of them
    in the lattice) after their sizes"""
    cl, lab, info = got
    rc, rl, ro, rn = ref
    assert [len(c) for c in cl] == [len(c) for c in rc]
    assert all(c.dtype == np.int32 for c in cl)
    if rc:
        np.testing.assert_array_equal(np.concatenate(cl), np.concatenate(rc))
    np.testing.assert_array_equal(lab, rl)
    np.testing.assert_array_equal(info["offsets"], ro)
    assert info["n_clusters"] == len(rc) and info["n_components"] == rn
    assert info["n_clustered_points"] == ro[-1]


def _check(eng, xyz, tol, mn=1, mx=0):
    got = eng.euclidean_clusters(xyz, tol, mn, mx)
    _assert_same(got, cc.ref_clusters(xyz, tol, mn, mx))
    return got


# ------------------------------------------------------------------------------- family A
@pytest.mark.parametrize("n_cells", [cc.A_CELLS, cc.A_CELLS_WIDE])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_linked_pairs_three_cells_apart(eng, axis, n_cells):
    """kCcReach: linked pairs whose computed cells are three apart on a line of 2^18 - 8 cells (with the
    same-cell shortcut) and of 2^20 - 8 cells (without) along each axis in turn (the cell decode differs
    per axis), beside twins one float step too far to link."""
    xyz, tol, pairs, twins = cc.reach_three(axis, n_cells)
    _, lab, info = _check(eng, xyz, tol)
    assert np.all(lab[pairs[:, 0]] == lab[pairs[:, 1]]) and np.all(lab[twins[:, 0]] != lab[twins[:, 1]])
    assert info["n_components"] == len(xyz) - len(pairs)


# ------------------------------------------------------------------------------- family B
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("step", ["linked", "apart"])
@pytest.mark.parametrize("arrangement", ["axis", "corner"])
def test_box_prune_at_one_float_step(eng, arrangement, step, mirrored):
    """cc_boxes_apart on a pair of cells of 130 x 70 points whose boxes' gap is the distance of one real
    pair of points: the largest float still linked (one cluster of 200) and one step further (130, 70)."""
    xyz, tol, _, _ = cc.box_prune(arrangement, step, mirrored)
    cl, _, _ = _check(eng, xyz, tol)
    assert [len(c) for c in cl] == ([200, 1] if step == "linked" else [130, 70, 1])


# ------------------------------------------------------------------------------- family C
@pytest.mark.parametrize("regime", ["shortcut", "wide", "widest", "clamped"])
def test_regime_switches(eng, regime):
    """The same-cell shortcut on a grid of 2^18 - 16 cells, none at 2^18 + 16, just under 2^20 and past
    the 2^20-cell clamp.  The witness is pair_tests on isolated populous cells: 0 with the shortcut, every
    pair of every cell without it."""
    w, tol = cc.regime_witness(regime)
    _, _, info = _check(eng, w, tol)
    assert info["pair_tests"] == cc.expected_pair_tests(w, tol)
    f, _ = cc.regime_full(regime)
    cl, _, _ = _check(eng, f, tol)
    assert [len(c) for c in cl][:4] == [200, 200, 130, 130]


def test_denormal_radius(eng):
    """float(tol^2) = 1e-40: denormal and not zero.  The pairs at 0.6e-20 link (their d2 is denormal too),
    those at 1.5e-20 do not."""
    xyz, tol = cc.denormal_radius()
    cl, _, info = _check(eng, xyz, tol)
    assert [len(c) for c in cl] == [2] * 100 + [1] * 300 and info["pair_tests"] > 0


def test_infinite_radius(eng):
    """float(tol^2) = +inf: every pair with a finite float d2 links, a pair whose d2 overflows does not"""
    xyz, tol = cc.infinite_radius()
    cl, _, _ = _check(eng, xyz, tol)
    assert [len(c) for c in cl] == [130, 1]


# ------------------------------------------------------------------------------- family D
@pytest.mark.parametrize("regime", ["wide", "clamped3", "clamped8"])
def test_populous_cells_without_shortcut(eng, regime):
    """Cells of 1, 2, 63, 64, 65, 129 and 200 points and neighbouring cells in both size orders on grids
    without the shortcut: the i < j pairing inside a cell and the larger-cell-on-the-lanes swap."""
    xyz, tol, _ = cc.populous_cells(regime)
    _, _, info = _check(eng, xyz, tol)
    assert 1 < info["n_components"] < len(xyz)


# ------------------------------------------------------------------------------- family E
@pytest.mark.parametrize("offset", list(OFFSETS))
def test_site_offsets_clusters(eng, offset):
    """the FOD cloud and the dense patch in site frames: coordinates of 300 m and 4096 m, moved in float32"""
    a = cc.site_fod(offset)
    for tol in cc.E_FOD_TOLS:
        fin_idx, comp = cc.site_fod_components(offset, tol)
        for mn, mx in cc.E_FOD_SIZES:
            got = eng.euclidean_clusters(a, tol, mn, mx)
            _assert_same(got, cc.finish(a, fin_idx, comp, mn, mx))
            assert got[1][7] == -1 and got[1][len(a) - 5] == -1  # the NaN and the Inf record
    # the dense patch: at site4096 the float spacing is half the tolerance
    _check(eng, cc.site_patch(offset), cc.E_PATCH_TOL)


@pytest.mark.parametrize("leaf,mp", cc.E_VOXEL_CONFIGS)
@pytest.mark.parametrize("offset", list(OFFSETS))
def test_site_offsets_voxel_grid(eng, offset, leaf, mp):
    """mgicp_voxel_grid in the same site frames; at leaf 10 one thread sums about 10 000 records in fp32"""
    from oracle import ref

    c = cc.site_rgb_cloud(offset)
    xyz_ref, rgba_ref, ovf = ref.voxel_grid(c.points, leaf, mp)
    assert not ovf
    out = eng.voxel_grid(c, leaf, mp)
    assert len(out) == len(xyz_ref)
    np.testing.assert_array_equal(out.xyz(), xyz_ref)
    np.testing.assert_array_equal(out.points["rgb"], rgba_ref)
    assert np.all(out.points["w"] == 1.0)


# ------------------------------------------------------------------------------- family F
def _contended(eng, xyz, tol):
    """three runs on one engine give one result, the reference's; a permuted copy gives the same sets"""
    ref = cc.ref_clusters(xyz, tol)
    for _ in range(3):
        _assert_same(eng.euclidean_clusters(xyz, tol), ref)
    perm = np.random.default_rng(71).permutation(len(xyz))
    cl, lab, info = eng.euclidean_clusters(np.ascontiguousarray(xyz[perm]), tol)
    assert [len(c) for c in cl] == [len(c) for c in ref[0]] and info["n_components"] == ref[3]
    # label of every original point: the same partition, cluster by cluster up to the order of equal sizes
    back = np.empty(len(xyz), np.int64)
    back[perm] = lab
    pairs = np.unique(np.stack([ref[1].astype(np.int64), back], 1), axis=0)
    assert len(pairs) == len(ref[0]) and len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])) == len(pairs)
    sizes = np.array([len(c) for c in ref[0]])
    assert np.array_equal(sizes[pairs[:, 0]], sizes[pairs[:, 1]])
    return ref


def test_lattice_forest(eng):
    xyz, tol_joined, tol_apart = cc.lattice32()
    ref = _contended(eng, xyz, tol_joined)
    assert [len(c) for c in ref[0]] == [32768]
    ref = _contended(eng, xyz, tol_apart)
    assert len(ref[0]) == 32768 and np.array_equal(ref[1], np.arange(32768))  # the tie rule: ascending


def test_comb_forest(eng):
    xyz, tol, cut = cc.comb()
    ref = _contended(eng, xyz, tol)
    assert [len(c) for c in ref[0]] == [6975, 25]
    np.testing.assert_array_equal(ref[0][1], np.arange(*cut))
