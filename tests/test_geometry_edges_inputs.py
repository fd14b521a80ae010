"""The inputs of tests/test_geometry_edges_gpu.py are what they claim (CPU, the oracle alone).

Each case of the GPU module is built to reach one regime of the grid searches' float reasoning; the
conditions those cases depend on are asserted here on the reference, never on the engine: duplicates and
ties really occur far from the origin, the gates really cut, the rotated pairs really overlap, the
degenerate neighbourhoods really give finite matrices, the void really is a void.
"""
import numpy as np
import pytest

import geometry_edges_cases as gc


def _accepted(o, T):
    m, tj, _, _ = o.correspondences(T)
    assert m == int((tj >= 0).sum())
    return m


def test_far_patch_has_duplicates_and_ties():
    """at 4096 m the float32 ulp (4.9e-4 m in x) is a third of the patch's 1.6 mm spacing"""
    src, tgt, _ = gc.far_pair("patch", "site4096")
    assert float(np.spacing(np.float32(4096.5))) == pytest.approx(4.8828125e-4)
    dup, tie = gc.duplicates_and_ties(src, 20)
    assert dup > 0 and tie > 0, (dup, tie)
    dup7, tie7 = gc.duplicates_and_ties(src, 7)
    assert tie7 > 0
    # the control has neither duplicates nor (more than a handful of) ties
    dup0, tie0 = gc.duplicates_and_ties(gc.far_pair("patch", "origin")[0], 20)
    assert dup0 == 0 and tie0 < tie


@pytest.mark.parametrize("offset", list(gc.OFFSETS))
def test_far_offsets_are_applied_in_float32(offset):
    for pair in gc.PAIRS:
        src, tgt, _ = gc.far_pair(pair, offset)
        assert src.dtype == np.float32 and tgt.dtype == np.float32
        off = np.asarray(gc.OFFSETS[offset])
        span = 5.0 if pair == "part" else 0.3
        assert np.abs(src.astype(np.float64).mean(0) - off).max() < span
        assert np.abs(tgt.astype(np.float64).mean(0) - off).max() < span


@pytest.mark.parametrize("offset", list(gc.OFFSETS))
def test_patch_gate_cuts(offset):
    """the oracle accepts between 10 % and 90 % of the patch at every transform of the sweeps"""
    src, tgt, gate = gc.far_pair("patch", offset)
    o = gc.oracle(src, tgt, max_corr_dist=gate)
    for T in gc.far_transforms("patch", offset):
        frac = _accepted(o, T) / len(src)
        assert 0.1 <= frac <= 0.9, (offset, frac)


@pytest.mark.parametrize("offset", list(gc.OFFSETS))
def test_part_sweeps_accept_and_reject(offset):
    """the part at the default gate: identity and the shift accept most points, the 0.3 rad turn about
    the cloud's centre keeps the points near the axis only -- all three accept and reject some"""
    src, tgt, gate = gc.far_pair("part", offset)
    o = gc.oracle(src, tgt, max_corr_dist=gate)
    fr = [_accepted(o, T) / len(src) for T in gc.far_transforms("part", offset)]
    assert fr[0] > 0.5 and fr[1] > 0.5, fr
    assert 0.02 < fr[2] < 0.9, fr
    assert all(f < 1.0 for f in fr), fr


@pytest.mark.parametrize("dist", gc.FAR_QUERY_DIST)
def test_far_queries_dwarf_the_targets_maxabs(dist):
    tgt = gc.centred_patch()
    src = gc.far_query_source(dist)
    assert np.abs(tgt).max() < 0.11
    assert np.abs(src).max() > 3.0 * np.abs(tgt).max()
    # the gated sweep (5 m) accepts everything at 0.5 m and 3 m, nothing at 40 m
    o = gc.oracle(src, tgt, max_corr_dist=5.0)
    m = _accepted(o, np.eye(4, dtype=np.float32))
    assert m == (len(src) if dist < 5.0 else 0)


@pytest.mark.parametrize("angle", gc.ROT_ANGLES)
def test_rotated_pairs_overlap(angle):
    src, tgt, T = gc.rotated_pair(angle)
    m = _accepted(gc.oracle(src, tgt), T)
    assert 0.5 * len(src) < m < len(src), m


def test_split_source_leaves_whole_chunks_unmatched():
    """2048 of the 4096 points are moved 0.5 m up and sort last (two whole chunks).  The part has
    structure half a metre above some of them, so a few (3) still find a partner -- all of them in the lower
    of the two moved chunks by z, the 1024 highest points are all rejected.  Of the 2048 left in place the
    gate accepts more than one chunk's worth but not all, so at least one of their chunks is partly filled."""
    src, tgt, Ttrue = gc.split_source()
    scan = gc.part20000()[0][:4096]
    moved = src[:, 2] != scan[:, 2]
    assert moved.sum() == 2 * gc.CHUNK_PTS
    assert src[moved, 2].min() - src[~moved, 2].max() > 0.4  # no grid layer holds both kinds
    m, tj, _, _ = gc.oracle(src, tgt).correspondences(np.linalg.inv(Ttrue).astype(np.float32))
    top = np.argsort(src[:, 2], kind="stable")[-gc.CHUNK_PTS:]
    assert (tj[top] < 0).all()
    assert src[tj >= 0, 2].max() < src[top, 2].min() - 0.05
    assert gc.CHUNK_PTS < (tj[~moved] >= 0).sum() < 2 * gc.CHUNK_PTS, m


@pytest.mark.parametrize("k", [20, 7])
def test_degenerate_covariances_are_finite(k):
    from oracle import ref

    for name, pts in gc.degenerate_clouds().items():
        c = ref.covariances(pts, k=k)
        assert np.isfinite(c).all(), name
        assert np.abs(c).max() > 0, name
    same = gc.degenerate_clouds()["same"]
    assert (same.max(0) == same.min(0)).all()  # zero extent


def test_dumbbell_void():
    tgt, q, groups = gc.dumbbell()
    assert len(tgt) == 16000 and len(q) == 2000
    d = np.sqrt(gc.nearest_d2_bruteforce(q, tgt).astype(np.float64))
    a, b = groups["ball"]
    assert d[a:b].min() > 0.5  # the midpoint queries: no target within half a metre
    a, b = groups["inside"]
    assert np.median(d[a:b]) < 0.01
    a, b = groups["faces"]
    lo, hi = tgt.min(0), tgt.max(0)
    assert ((q[a:b] < lo) | (q[a:b] > hi)).any(axis=1).all()  # every one of them outside the bbox
    # the 4 cm gate decides both ways among the queries
    m = _accepted(gc.oracle(q, tgt, max_corr_dist=gc.DUMBBELL_GATE), np.eye(4, dtype=np.float32))
    assert 0.1 * len(q) < m < 0.9 * len(q), m


def test_oracle_set_source_rejects_bad_arguments():
    """ref_set_source validates before it touches the handle: REF_E_INVALID, not a crash"""
    from oracle import ref

    lib = ref.load()
    pts = np.zeros((4, 3), np.float32)
    assert lib.ref_set_source(None, pts.ctypes.data, 4, 12) != 0
    o = ref.RefGICP()
    assert lib.ref_set_source(o.h, None, 4, 12) != 0
    assert lib.ref_set_source(o.h, pts.ctypes.data, 4, 8) != 0
    assert o.set_source(pts) == 0
