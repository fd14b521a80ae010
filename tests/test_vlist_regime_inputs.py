"""CPU side of the 1-NN cell-list regime tests: the premises of tests/vlist_regime_cases.py that do not
depend on the engine's grid (the GPU side asserts the rest from GICPEngine.vlist_layout)."""
import numpy as np
import pytest

import vlist_regime_cases as vc

# 0.6 h for any h the grid sizing may pick: the 5 mm sheet (h of 3..17 mm), the 20k part (~28 mm between
# neighbours: h of 17..80 mm)
PLAUSIBLE_C = {"probe": (0.002, 0.003, 0.0047, 0.006, 0.01), "part": (0.01, 0.017, 0.03, 0.05)}


def _oracle(tgt, src, gate=vc.GATE):
    from oracle import ref

    o = ref.RefGICP(max_corr_dist=gate)
    o.set_source(src)
    o.set_target(tgt)
    return o


@pytest.mark.parametrize("kind,n", [("dup", 512), ("dup", 513), ("dup", 1024), ("dup", 1025), ("clump", 700),
                                    ("clump", 3000)])
def test_probe_premises(kind, n):
    tgt = (vc.dup_target if kind == "dup" else vc.clump_target)(n)
    src, roles = vc.probe_source()
    P = vc.point_p().astype(np.float64)
    nsheet = len(vc.sheet())
    assert len(tgt) == nsheet + n and np.array_equal(tgt[:nsheet], vc.sheet())
    # every other target point lies farther than 3 gates from P
    assert np.linalg.norm(tgt[:nsheet].astype(np.float64) - P, axis=1).min() > 3 * vc.GATE
    extra = tgt[nsheet:]
    if kind == "dup":
        assert (extra == vc.point_p()).all()
    else:  # distinct floats, all within the clump's ball (and a float step of its rim)
        assert len(np.unique(extra, axis=0)) == n
        assert np.linalg.norm(extra.astype(np.float64) - P, axis=1).max() <= vc.CLUMP_R + 1e-6
    assert (roles == 0).sum() == 2300 and (roles == 1).sum() == 500 and (roles == 2).sum() == nsheet
    d = np.linalg.norm(src.astype(np.float64) - P, axis=1)
    assert d[roles == 0].max() <= vc.BALL_R + 1e-6
    assert (d[roles == 0] <= vc.CORE_R + 1e-6).sum() >= 300
    assert d[roles == 1].min() >= vc.SHELL_R[0] - 1e-6 and d[roles == 1].max() <= vc.SHELL_R[1] + 1e-6
    o = _oracle(tgt, src)
    for T in vc.probe_transforms():
        m, tj, _, _ = o.correspondences(T)
        assert (tj[roles == 0] >= 0).sum() > 1500
        assert (tj[roles == 1] < 0).any() and (tj[roles == 1] >= 0).any()
        if kind == "dup":  # the winner among the copies: their lowest original index
            assert set(np.unique(tj[roles == 0])) <= {-1, nsheet}
        assert (tj[roles == 2] >= 0).all() and (tj[roles == 2] < nsheet).all()


@pytest.mark.parametrize("which,c", [(w, c) for w, cs in PLAUSIBLE_C.items() for c in cs])
def test_queries_stay_clear_of_cell_faces(which, c):
    """the regime certification leaves out queries within es of a cell face and asserts that they are at
    most 10 %: for any plausible fine cell the cases' queries are far inside that cap (uniform queries:
    a share of about 6 es / c, 2.5 % at the smallest cell here; half the cap is asserted)"""
    src, _ = vc.probe_source()
    cases = {"probe": [(vc.dup_target(1024), src, vc.GATE), (vc.clump_target(3000), src, vc.GATE)],
             "part": [(vc.part()[1], vc.volume_source(g), g) for g in vc.VOLUME_GATES]}
    for tgt, q, gate in cases[which]:
        es = vc.es_of(tgt, gate, c)
        assert es < 0.01 * c
        pad = gate * (1.0 + 1e-5) + 1e-9 + 2.0 * c
        o = tgt.astype(np.float64).min(0) - pad
        assert vc.near_face_share(q, o, c, es) <= 0.05


def test_volume_sources():
    cad = vc.part()[1].astype(np.float64)
    assert len(cad) <= 25000
    for g in vc.VOLUME_GATES:
        q = vc.volume_source(g).astype(np.float64)
        assert len(q) == 20000
        assert (q >= cad.min(0) - g - 1e-6).all() and (q <= cad.max(0) + g + 1e-6).all()
        # off-surface: most queries are farther than 5 mm from every target point (the scans of the other
        # list tests lie within the 0.5 mm noise of the surface)
        o = _oracle(vc.part()[1], vc.volume_source(g), gate=0.005)
        m, _, _, _ = o.correspondences(np.eye(4, dtype=np.float32))
        assert m < 0.2 * len(q)


def test_pool_range_helpers():
    assert vc.padded([0, 1, 4, 5, 62, 63, 64, 512, 513, 1024]).tolist() == [0, 4, 4, 8, 64, 68, 68, 516, 520, 1028]
    st = np.array([vc.LISTED, vc.REJECT, vc.LISTED, vc.LISTED, vc.OVERFLOW], np.uint8)
    ln = np.array([5, 0, 63, 4, 0], np.uint32)
    of = np.array([0, 0, 8, 76, 0], np.uint32)
    assert vc.pool_ranges_ok(st, ln, of, 80) == (True, True)
    assert vc.pool_ranges_ok(st, ln, of, 79) == (False, True)
    of[3] = 72  # inside the long list's padded range [8, 76)
    assert vc.pool_ranges_ok(st, ln, of, 80) == (True, False)


def test_cell_mapping_and_corner_queries():
    lay = {"ox": 1.0, "oy": 2.0, "oz": -0.5, "c": 0.25, "inv_c": 4.0, "es": 0.001, "nx": 8, "ny": 4, "nz": 4}
    q = np.array([[1.1, 2.1, -0.4], [1.6, 2.3, 0.1], [0.9, 2.1, -0.4], [1.2505, 2.1, -0.4]])
    ci, inside, near = vc.cell_index(lay, q)
    assert ci[:2].tolist() == [0, 2 + 8 * (1 + 4 * 2)] and inside.tolist() == [True, True, False, True]
    assert near.tolist() == [False, False, False, True]
    ci32, in32 = vc.cell_index_f32(lay, q)
    assert ci32[:2].tolist() == ci[:2].tolist() and in32.tolist() == inside.tolist()
    cq = vc.corner_queries(lay, [2 + 8 * (1 + 4 * 2)]).astype(np.float64)
    assert cq.shape == (37, 3)
    lo, hi = np.array([1.5, 2.25, 0.0]), np.array([1.75, 2.5, 0.25])
    on_corner = ((cq == lo) | (cq == hi)).all(1)
    assert on_corner.sum() == 8
    # nudged corners: one float step off a corner in every coordinate, 8 strictly inside, 8 strictly outside
    step = (np.abs(cq[:, None, :] - np.stack([lo, hi])[None]).min(1) <= 3e-7).all(1) & ~on_corner
    assert step.sum() == 16
    strictly_in = ((cq > lo) & (cq < hi)).all(1)
    assert (step & strictly_in).sum() == 8
    outside = ((cq < lo) | (cq > hi)).any(1)
    assert (outside & ~step).sum() == 6  # es / 2 outside each face
    d = np.maximum(lo - cq, cq - hi).max(1)[outside & ~step]
    np.testing.assert_allclose(d, 0.0005, rtol=1e-3)
    assert np.isclose(cq, 0.5 * (lo + hi)).all(1).sum() == 1


def test_transform_model_and_gates():
    src, _ = vc.probe_source()
    I, S = vc.probe_transforms()
    assert np.array_equal(vc.xform32(I, src), src)
    assert np.array_equal(vc.xform32(S, src), src + S[:3, 3])
    assert vc.PCL_DEFAULT_GATE > 1e154 and np.isfinite(vc.PCL_DEFAULT_GATE ** 2)
