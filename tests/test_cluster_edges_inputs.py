"""The inputs of the clustering / voxel-grid edge tests are what they claim to be (CPU only).

Every cloud of tests/cluster_edges_cases.py is checked twice: the property that makes it an edge case
holds (computed cells three apart, a one-float-step flip, the cell populations, the grid's regime),
and the reference that tests/test_cluster_edges_gpu.py compares the engine with agrees with an
all-pairs brute force on it -- on the whole cloud up to about 1500 points, on a subset otherwise.
"""
import numpy as np
import pytest

import cluster_edges_cases as cc
from geometry_edges_cases import OFFSETS, d2_rows

MiB = 1 << 20


def _ref_is_bruteforce(xyz, tol, sizes=((1, 0),)):
    assert len(xyz) <= 1600
    for mn, mx in sizes:
        assert cc.same_result(cc.ref_clusters(xyz, tol, mn, mx), cc.bruteforce_clusters(xyz, tol, mn, mx))


# ------------------------------------------------------------------------------- family A
@pytest.mark.parametrize("n_cells", [cc.A_CELLS, cc.A_CELLS_WIDE])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_reach_three_pairs(axis, n_cells):
    xyz, tol, pairs, twins = cc.reach_three(axis, n_cells)
    g = cc.grid_of(xyz, tol)
    want = [1, 1, 1]
    want[axis] = n_cells
    assert g.dims == want and g.h == 0.5 * tol and g.table_bytes <= 4.01 * MiB
    assert g.shortcut == (n_cells == cc.A_CELLS) and (g.table_bytes <= 1.01 * MiB or not g.shortcut)
    assert abs(float(g.o[axis])) > 100  # an origin far from zero
    c = g.cells(xyz)[:, axis]
    assert len(pairs) >= 100 and len(twins) >= len(pairs) // 2
    assert np.all(np.abs(c[pairs[:, 0]] - c[pairs[:, 1]]) == 3)
    r2 = cc.r2_of(tol)
    assert np.all(cc.d2_f32(xyz[pairs[:, 0]], xyz[pairs[:, 1]]) < r2)
    # the twins: one float step further, not linked
    tb = xyz[twins[:, 1]].copy()
    assert np.all(cc.d2_f32(xyz[twins[:, 0]], tb) >= r2)
    tb[:, axis] = np.nextafter(tb[:, axis], xyz[twins[:, 0], axis])
    assert np.all(cc.d2_f32(xyz[twins[:, 0]], tb) < r2)
    # groups at least 20 cells from each other
    cs = np.sort(c)
    gaps = np.diff(cs)
    assert np.all((gaps <= 3) | (gaps >= 20))
    # the partition: every pair one cluster of two, every other point alone
    cl, lab, _, ncomp = cc.ref_clusters(xyz, tol)
    assert ncomp == len(xyz) - len(pairs) and [len(x) for x in cl[:len(pairs)]] == [2] * len(pairs)
    assert np.all(lab[pairs[:, 0]] == lab[pairs[:, 1]]) and np.all(lab[twins[:, 0]] != lab[twins[:, 1]])
    _ref_is_bruteforce(xyz, tol)


# ------------------------------------------------------------------------------- family B
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("arrangement", ["axis", "corner"])
def test_box_prune_flips_at_one_float_step(arrangement, mirrored):
    lk, tol, ia, ib = cc.box_prune(arrangement, "linked", mirrored)
    ap, _, _, _ = cc.box_prune(arrangement, "apart", mirrored)
    r2 = cc.r2_of(tol)
    na, nb = cc.B_NA, cc.B_NB
    assert na * nb >= cc.BOX_MIN_PAIRS and len(lk) == len(ap) == 1 + na + nb
    # A's extreme point is the last of its cell in input (= sorted) order, B's in the middle of its own
    assert ia - 1 == na - 1 >= 128 and ib - 1 - na == 35
    moved = np.flatnonzero((lk != ap).any(1))
    assert list(moved) == [ib]
    last = 2 if arrangement == "corner" else 0
    away = np.float32(np.inf) if not mirrored else -np.float32(np.inf)
    assert np.nextafter(lk[ib, last], away) == ap[ib, last] and np.array_equal(np.delete(lk[ib], last), np.delete(ap[ib], last))
    for xyz, linked in ((lk, True), (ap, False)):
        g, keys, counts = cc.cell_counts(xyz, tol)
        assert g.shortcut and np.all(xyz[0] == 0)
        A, B = xyz[1:1 + na], xyz[1 + na:]
        ca, cb = np.unique(g.cells(A), axis=0), np.unique(g.cells(B), axis=0)
        assert len(ca) == 1 and len(cb) == 1 and sorted(counts) == [1, nb, na]  # nobody in the cells between
        step = (cb - ca)[0]
        sign = -2 if mirrored else 2
        assert list(step) == ([sign] * 3 if arrangement == "corner" else [sign, 0, 0])
        ka, kb = g.keys(A)[0], g.keys(B)[0]
        assert (kb < ka) == mirrored  # mirrored: B is the earlier cell of the pair
        # the boxes' gap is the extreme pair's distance, in the kernel's own float expression
        G = cc.box_gap_f32(A, B)
        assert G == cc.d2_f32(xyz[ia], xyz[ib])
        assert (G < r2) == linked
        assert np.float32(G * np.float32(0.99999)) < r2  # the prune must not fire on either side
        if arrangement == "axis":  # the clumps overlap on y and z
            for d in (1, 2):
                assert A[:, d].min() < B[:, d].max() and B[:, d].min() < A[:, d].max()
        cross = cc.d2_f32(A[:, None, :], B[None, :, :]) < r2
        assert cross.sum() == (1 if linked else 0) and cross[na - 1, 35] == linked  # the only link there is
        sizes = [len(c) for c in cc.ref_clusters(xyz, tol)[0]]
        assert sizes == ([na + nb, 1] if linked else [na, nb, 1])
        _ref_is_bruteforce(xyz, tol)


# ------------------------------------------------------------------------------- family C
C_DIMS = {"shortcut": (1 << 18) - 16, "wide": (1 << 18) + 16, "widest": (1 << 20) - 16}


@pytest.mark.parametrize("regime", ["shortcut", "wide", "widest", "clamped"])
def test_regime_clouds(regime):
    w, tol = cc.regime_witness(regime)
    f, _ = cc.regime_full(regime)
    for xyz in (w, f):
        g = cc.grid_of(xyz, tol)
        assert g.dims[1:] == [1, 1] and g.table_bytes < 8 * MiB
        assert g.shortcut == (regime == "shortcut")
        if regime == "clamped":
            assert g.dims[0] in (1 << 20, (1 << 20) + 1) and 1.49 * cc.C_H < g.h < 1.51 * cc.C_H
        else:
            assert g.dims[0] == C_DIMS[regime] and g.h == cc.C_H
    # the witness: isolated populous cells with the counts they were built with, and the two anchors
    g, _, counts = cc.cell_counts(w, tol)
    assert sorted(counts) == sorted([1, 1] + [n for _, n in cc.C_ISOLATED])
    assert cc.occupied_cells_isolated(w, tol)
    want = cc.expected_pair_tests(w, tol)
    assert (want == 0) == (regime == "shortcut")
    if regime != "shortcut":
        assert want == sum(n * (n - 1) // 2 for _, n in cc.C_ISOLATED)
    sizes = [len(c) for c in cc.ref_clusters(w, tol)[0]]
    assert sizes == sorted([n for _, n in cc.C_ISOLATED], reverse=True) + [1, 1]
    _ref_is_bruteforce(w, tol)
    # the full cloud adds the clumps in both steps and both cell orders
    sizes = [len(c) for c in cc.ref_clusters(f, tol)[0]]
    assert sizes[:4] == [200, 200, 130, 130] and sizes.count(70) == 2
    if regime != "clamped":  # cells of tol / 2: the clumps' pairs of cells reach the box test
        _, _, counts = cc.cell_counts(f, tol)
        assert sorted(counts)[-4:] == [130] * 4 and list(counts).count(70) == 4
    _ref_is_bruteforce(f, tol)


def test_denormal_radius_cloud():
    xyz, tol = cc.denormal_radius()
    r2 = cc.r2_of(tol)
    assert 0 < r2 < cc.TINY32  # denormal, not zero
    g = cc.grid_of(xyz, tol)
    assert not g.shortcut and max(g.dims) <= 201
    assert np.all(cc.d2_f32(xyz[:100], xyz[300:400]) < r2)
    assert np.all(cc.d2_f32(xyz[100:200], xyz[400:500]) >= r2)
    assert np.all(cc.d2_f32(xyz[:100], xyz[300:400]) > 0)  # the linked pairs' d2 are denormal themselves
    cl, lab, _, ncomp = cc.ref_clusters(xyz, tol)
    sizes = [len(c) for c in cl]
    assert ncomp == 400 and sizes == [2] * 100 + [1] * 300
    assert np.array_equal(lab[:100], lab[300:400])
    _ref_is_bruteforce(xyz, tol)


def test_infinite_radius_cloud():
    xyz, tol = cc.infinite_radius()
    assert np.isinf(cc.r2_of(tol)) and not cc.grid_of(xyz, tol).shortcut
    d2 = cc.d2_f32(xyz[:, None, :], xyz[None, :, :])
    assert np.isinf(d2).any() and np.isfinite(d2).sum() > len(xyz)  # both outcomes occur
    assert [len(c) for c in cc.ref_clusters(xyz, tol)[0]] == [130, 1]
    _ref_is_bruteforce(xyz, tol)


# ------------------------------------------------------------------------------- family D
@pytest.mark.parametrize("regime", ["wide", "clamped3", "clamped8"])
def test_populous_cells(regime):
    xyz, tol, want = cc.populous_cells(regime)
    g, keys, counts = cc.cell_counts(xyz, tol)
    assert not g.shortcut and g.dims[1:] == [1, 1] and g.table_bytes < 8 * MiB
    got = dict(zip(keys.tolist(), counts.tolist()))
    assert {c: got.get(c) for c in want} == want and len(got) == len(want) + 2
    assert sorted(n for n in want.values()) == sorted(list(cc.D_SIZES) + [n for p in cc.D_NEIGHBOURS for n in p])
    # the neighbouring cells, in both size orders
    order = [(want[c], want[c + 1]) for c in sorted(want) if c + 1 in want]
    assert order == list(cc.D_NEIGHBOURS)
    # the share of linked pairs inside the populous cells
    c = g.cells(xyz)[:, 0]
    r2 = cc.r2_of(tol)
    for cell, n in want.items():
        if n >= 63:
            p = xyz[c == cell]
            share = ((cc.d2_f32(p[:, None, :], p[None, :, :]) < r2).sum() - n) / (n * (n - 1))
            lo, hi = {"wide": (1.0, 1.0), "clamped3": (0.4, 0.7), "clamped8": (0.03, 0.12)}[regime]
            assert lo <= share <= hi, (cell, n, share)
    ncomp = cc.ref_clusters(xyz, tol)[3]
    assert 1 < ncomp < len(xyz)
    if regime == "clamped8":
        assert ncomp > len(want)  # cells fall apart into several components
    _ref_is_bruteforce(xyz, tol)


# ------------------------------------------------------------------------------- family E
@pytest.mark.parametrize("offset", list(OFFSETS))
def test_site_clouds(offset):
    f = cc.site_fod(offset)
    assert np.isnan(f[7]).all() and np.isinf(f[len(f) - 5, 1]) and np.isfinite(f).all(1).sum() == len(f) - 2
    sub = f[:1500]
    for tol in cc.E_FOD_TOLS:
        _ref_is_bruteforce(sub, tol, cc.E_FOD_SIZES)
        ncomp = cc.ref_clusters(f, tol)[3]
        assert 1 < ncomp < len(f)
    p = cc.site_patch(offset)
    _ref_is_bruteforce(p[:1500], cc.E_PATCH_TOL)
    if offset == "site4096":
        # x near 4096.5: floats 2^-11 = 4.9e-4 apart, half the tolerance -- exact duplicates, and pairs at
        # exactly two float steps (d2 = 2^-20 < float(tol^2): linked by a tie-heavy margin)
        two = np.float32(np.float32(2.0 ** -10) ** 2)
        assert two < cc.r2_of(cc.E_PATCH_TOL)
        dup = twostep = 0
        for _, d2 in d2_rows(p, p):
            dup += int((d2 == 0).sum()) - len(d2)
            twostep += int((d2 == two).sum())
        assert dup >= 2 and twostep >= 2


@pytest.mark.parametrize("offset", list(OFFSETS))
def test_site_voxel_oracle_matches_bruteforce(offset):
    from oracle import ref
    from test_fod_filters import _bruteforce_voxels

    c = cc.site_rgb_cloud(offset, 3000)
    assert np.isnan(c.points["x"][5]) and np.isinf(c.points["y"][17])
    for leaf, mp in cc.E_VOXEL_CONFIGS:
        xyz, rgba, ovf = ref.voxel_grid(c.points, leaf, mp)
        bx, bc = _bruteforce_voxels(c.points, leaf, mp)
        assert not ovf and len(xyz) > 0
        np.testing.assert_array_equal(xyz, bx)
        np.testing.assert_array_equal(rgba, bc)
        if leaf == 10.0:  # almost the whole cloud in two leaves
            assert len(xyz) <= 4


# ------------------------------------------------------------------------------- family F
def test_lattice_and_comb():
    xyz, tol_joined, tol_apart = cc.lattice32()
    assert len(xyz) == 32768 and tol_joined > tol_apart
    assert np.nextafter(cc.r2_of(tol_apart), np.float32(np.inf)) == cc.r2_of(tol_joined)
    cl, lab, _, ncomp = cc.ref_clusters(xyz, tol_joined)
    assert ncomp == 1 and len(cl[0]) == 32768
    cl, lab, _, ncomp = cc.ref_clusters(xyz, tol_apart)
    assert ncomp == 32768 and np.array_equal(lab, np.arange(32768))  # singletons in ascending order
    sub = xyz[np.lexsort(xyz.T)][:1024]  # a 32 x 32 sheet of the lattice
    for tol in (tol_joined, tol_apart):
        _ref_is_bruteforce(sub, tol)
    assert cc.ref_clusters(sub, tol_joined)[3] == 1 and cc.ref_clusters(sub, tol_apart)[3] == 1024
    xyz, tol, cut = cc.comb()
    cl, _, _, ncomp = cc.ref_clusters(xyz, tol)
    assert len(xyz) == 7000 and ncomp == 2 and [len(c) for c in cl] == [6975, 25]
    np.testing.assert_array_equal(cl[1], np.arange(*cut))
    # the cut tooth with its stretch of the spine: all pairs
    tooth = np.concatenate([xyz[1100:1180], xyz[cut[0] - 25:cut[1]]])
    _ref_is_bruteforce(tooth, tol)
    assert cc.ref_clusters(tooth, tol)[3] == 2
