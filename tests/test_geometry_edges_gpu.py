"""GPU parity at the edges of the grid searches' float reasoning (engine vs the CPU oracle).

Every result of the engine rests on the grid searches being exact (ring_search, box_search,
box_search_lds, the wave k-NN, the cell lists, empty_reject): FLANN's float L2_Simple order, ties broken
by the original index.  That is proved with a handful of float margins -- the grid's rounding slack
(8 ulps of the cloud's largest coordinate + 1e-6 cell), the 0.99999 / 1.00001 factors, cell_gap, the
clamp of the query cell index, the capped empty-space map -- which the rest of the suite only meets
where they are comfortable.  The families below reach the regimes it leaves out:

  1. clouds hundreds and thousands of metres from the origin (a few float levels per point spacing);
  2. queries much larger than the target's largest coordinate (the slack comes from the target alone);
  3. rotations up to pi in the sweeps, the objective and the moments;
  4. source sizes around the 64-lane wave and the 1024-point chunk, odd target sizes, empty chunks;
  5. rank-0 / rank-1 neighbourhoods and a zero-extent cloud;
  6. queries deep inside a void of the target's bbox, far beyond the empty-space map's cap.

Bars (tests/test_gicp_gpu.py's): counts and index arrays equal; covariances and Mahalanobis upper
triangles <= 1e-12 of the reference's max, covariance rows bit-identical for > 0.99 of the points;
objective |f - f_ref| <= 1e-10 |f_ref|, gradient <= 1e-9 max(1, max|g_ref|); fitness <= 1e-9 relative;
keep masks exact; moments 1e-10 of their block's scale (tests/test_gn_solver.py's).  The clouds are built
and their premises checked on the oracle in tests/geometry_edges_cases.py / test_geometry_edges_inputs.py.
"""
import numpy as np
import pytest

import geometry_edges_cases as gc
from conftest import frob

pytestmark = pytest.mark.gpu

FROB_TOL = 1e-4  # the north-star bar
FAR = [(p, o) for p in gc.PAIRS for o in gc.OFFSETS]
I4 = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def engine_mod():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    return GICPEngine


def _upper(M9):
    M = M9.reshape(-1, 3, 3)
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], axis=1)


def _engine(GICPEngine, src, tgt, **kw):
    e = GICPEngine(**kw)
    e.set_source_xyz(src)
    e.set_target_xyz(tgt)
    return e


def _check_cov(c_gpu, c_ref, what):
    err = np.abs(c_gpu - c_ref).max() / np.abs(c_ref).max()
    exact = float(np.mean(np.all(c_gpu == c_ref, axis=1)))
    print(f"{what}: covariance error {err:.3e} of max, bit-identical rows {exact:.4f}")
    assert err <= 1e-12, (what, err)
    assert exact > 0.99, f"{what}: only {exact:.4f} of covariances bit-identical"


def _check_sweep(o, e, T, seeded=False, what=""):
    """one sweep at T on both sides: count, indices, Mahalanobis; returns the oracle's (m, indices)"""
    m_ref, tj_ref, _, M_ref = o.correspondences(T)
    sweep = e.debug_correspondences_seeded if seeded else e.debug_correspondences
    m_gpu, tj_gpu, M_gpu = sweep(T, len(tj_ref))
    bad = np.flatnonzero(tj_gpu != tj_ref)
    if len(bad):
        print(f"{what}: {len(bad)} indices differ, first at source {bad[0]}: engine {tj_gpu[bad[0]]} oracle {tj_ref[bad[0]]}")
    assert m_gpu == m_ref, (what, m_gpu, m_ref)
    np.testing.assert_array_equal(tj_gpu, tj_ref, err_msg=what)
    ok = tj_ref >= 0
    if ok.any():
        Mu = _upper(M_ref)[ok]
        rel = np.abs(M_gpu[ok] - Mu).max() / np.abs(Mu).max()
        assert rel <= 1e-12, (what, rel)
    return m_ref, tj_ref, M_gpu


def _check_fdf(o, e, x, what=""):
    f_ref, g_ref = o.fdf(x)
    f_gpu, g_gpu = e.debug_fdf(x)
    assert f_ref != 0.0, what  # a relative bar needs a residual
    ef = abs(f_gpu - f_ref) / abs(f_ref)
    eg = np.abs(g_gpu - g_ref).max() / max(1.0, np.abs(g_ref).max())
    print(f"{what}: f {f_ref:.6e} relative error {ef:.3e}; gradient max {np.abs(g_ref).max():.3e} error {eg:.3e}")
    assert abs(f_gpu - f_ref) <= 1e-10 * abs(f_ref), (what, f_gpu, f_ref)
    assert np.abs(g_gpu - g_ref).max() <= 1e-9 * max(1.0, np.abs(g_ref).max()), (what, g_gpu, g_ref)


def _check_moments(o, e, T, m_ref, what=""):
    mo_ref = o.moments(T)
    mo_gpu = e.debug_moments(T)
    assert mo_gpu[73] == mo_ref[73] == m_ref, what
    assert np.all(mo_gpu[74:] == 0)
    for lo, hi in ((0, 1), (1, 13), (13, 73)):  # per-block scale: S0, B, Q
        scale = np.abs(mo_ref[lo:hi]).max()
        err = np.abs(mo_gpu[lo:hi] - mo_ref[lo:hi]).max()
        print(f"{what}: moments [{lo}, {hi}) error {err / scale if scale else err:.3e} of scale")
        np.testing.assert_allclose(mo_gpu[lo:hi], mo_ref[lo:hi], rtol=0, atol=1e-10 * scale, err_msg=what)


def _check_fitness(o, e, T, what="", **kw):
    f_ref, f_gpu = o.fitness(T, **kw), e.fitness(T, **kw)
    assert abs(f_gpu - f_ref) <= 1e-9 * f_ref, (what, f_gpu, f_ref)


def _moved_points(T, p):
    T = np.asarray(T, np.float64)
    return np.asarray(p, np.float64) @ T[:3, :3].T + T[:3, 3]


# ============================================================== family 1: far from the origin
@pytest.mark.parametrize("k", [20, 7])
@pytest.mark.parametrize("pair,offset", FAR)
def test_far_covariances(engine_mod, pair, offset, k):
    from oracle import ref

    src, tgt, _ = gc.far_pair(pair, offset)
    e = _engine(engine_mod, src, tgt, k=k)
    for which, pts in (("source", src), ("target", tgt)):
        _check_cov(e.debug_covariances(which, len(pts)), ref.covariances(pts, k=k), f"{pair} {offset} {which} k={k}")
    e.close()


@pytest.mark.parametrize("pair,offset", FAR)
def test_far_sweeps_cold_and_seeded(engine_mod, pair, offset):
    """cold sweeps at I, a few-millimetre shift and a 0.3 rad turn about the cloud's centre, then the same
    three as a seeded sequence"""
    src, tgt, gate = gc.far_pair(pair, offset)
    Ts = gc.far_transforms(pair, offset)
    o = gc.oracle(src, tgt, max_corr_dist=gate)
    e = _engine(engine_mod, src, tgt, max_corr_dist=gate)
    for i, T in enumerate(Ts):
        _check_sweep(o, e, T, what=f"{pair} {offset} cold {i}")
    for i, T in enumerate(Ts + Ts[::-1]):
        _check_sweep(o, e, T, seeded=True, what=f"{pair} {offset} seeded {i}")
    e.close()
    # a seeded sequence straight after one cold sweep (the seeds come from the r03 sweep, not the lists)
    e = _engine(engine_mod, src, tgt, max_corr_dist=gate)
    _check_sweep(o, e, Ts[0], what=f"{pair} {offset} cold")
    for i, T in enumerate(Ts):
        _check_sweep(o, e, T, seeded=True, what=f"{pair} {offset} seeded after one {i}")
    e.close()


@pytest.mark.parametrize("pair,offset", FAR)
def test_far_cell_list_sweeps(engine_mod, pair, offset):
    """each transform three times in a row (lists requested, built, used), against the oracle and against
    the engine without cell lists, Mahalanobis matrices bit for bit between the two engines"""
    src, tgt, gate = gc.far_pair(pair, offset)
    o = gc.oracle(src, tgt, max_corr_dist=gate)
    e = _engine(engine_mod, src, tgt, max_corr_dist=gate, options={"vlist_eager": 0, "vlist_cold": 0})
    e0 = _engine(engine_mod, src, tgt, max_corr_dist=gate, options={"vlist_eager": 0, "vlist_cold": 0, "vlist": 0})
    stats = []
    for i, T in enumerate(gc.far_transforms(pair, offset)):
        for rep in range(3):
            what = f"{pair} {offset} T{i} rep {rep}"
            _, tj_ref, M = _check_sweep(o, e, T, what=what + " lists")
            _, _, M0 = _check_sweep(o, e0, T, what=what + " no lists")
            np.testing.assert_array_equal(M, M0, err_msg=what)
            stats.append(e.vlist_stats())
    assert e0.vlist_stats()["cells"] == 0
    assert stats[0]["requested"] == 0 and stats[1]["requested"] > 0, stats[:2]
    for k in (2, 5, 8):  # the third identical sweep finds every cell listed or rejected
        assert stats[k]["requested"] == 0, (k, stats[k])
        assert stats[k]["pending"] <= stats[k]["overflow"] * 64, (k, stats[k])
    assert stats[2]["lists"] > 0
    e.close()
    e0.close()


@pytest.mark.parametrize("pair,offset", FAR)
def test_far_fitness(engine_mod, pair, offset):
    src, tgt, gate = gc.far_pair(pair, offset)
    o = gc.oracle(src, tgt, max_corr_dist=gate)
    e = _engine(engine_mod, src, tgt, max_corr_dist=gate)
    for i, T in enumerate(gc.far_transforms(pair, offset)):
        _check_fitness(o, e, T, what=f"{pair} {offset} T{i}")
        f_ref = o.fitness(T)
        f6_ref, f6_gpu = o.fitness(T, max_range=1e-6), e.fitness(T, max_range=1e-6)
        assert abs(f6_gpu - f6_ref) <= 1e-9 * f_ref, (pair, offset, i, f6_gpu, f6_ref)
    e.close()


@pytest.mark.parametrize("pair,offset", FAR)
def test_far_objective(engine_mod, pair, offset):
    """the objective at three states after a gated sweep at the shift, and the moments there"""
    src, tgt, gate = gc.far_pair(pair, offset)
    T = gc.far_transforms(pair, offset)[1]
    o = gc.oracle(src, tgt, max_corr_dist=gate)
    e = _engine(engine_mod, src, tgt, max_corr_dist=gate)
    m_ref, _, _ = _check_sweep(o, e, T, what=f"{pair} {offset}")
    assert 0 < m_ref < len(src)
    for i, x in enumerate(gc.FDF_STATES):
        _check_fdf(o, e, np.array(x), what=f"{pair} {offset} state {i}")
    e.close()


@pytest.mark.parametrize("pair,offset", FAR)
def test_far_segment_differences(engine_mod, pair, offset):
    from leica_point_cloud_processing_amd import synth
    from oracle import ref

    src, tgt, _ = gc.far_pair(pair, offset)
    thr = gc.segment_threshold(pair)
    e = engine_mod()
    keep_ref, cnt_ref = ref.segment_differences(src, tgt, thr)
    keep, cnt = e.segment_differences(src, tgt, thr)
    np.testing.assert_array_equal(keep, keep_ref)
    assert cnt == cnt_ref and 0 < cnt_ref < len(src)
    for T in gc.far_transforms(pair, offset)[1:]:
        keep_ref, cnt_ref = ref.segment_differences(synth.transform_points(T, src), tgt, thr)
        keep, cnt = e.segment_differences(src, tgt, thr, T=T)
        np.testing.assert_array_equal(keep, keep_ref)
        assert cnt == cnt_ref and 0 < cnt_ref < len(src)
    e.close()


@pytest.mark.parametrize("pair,offset", FAR)
def test_far_resolution_and_radius_filter(engine_mod, pair, offset):
    src, _, _ = gc.far_pair(pair, offset)
    e = engine_mod()
    res_ref = gc.resolution_bruteforce(src)
    res = e.cloud_resolution(src)
    assert abs(res - res_ref) <= 1e-9 * res_ref, (res, res_ref)
    radius = 2.0 * res_ref
    keep_ref = gc.radius_keep_bruteforce(src, radius, 3)
    keep = e.radius_filter(src, radius, 3)
    np.testing.assert_array_equal(keep, keep_ref)
    assert 0 < keep_ref.sum() < len(src)
    e.close()


@pytest.mark.parametrize("pair,offset", FAR)
def test_far_align(engine_mod, pair, offset):
    """one align per pair and offset: converged flag and iterations equal, and the two transforms send
    every source point to the same place within 1e-4 m (the north-star bar as it applies to a site frame:
    the translation's own float32 ulp is 4.9e-4 at 4096 m, so the raw Frobenius difference means nothing)"""
    src, tgt, gate = gc.far_pair(pair, offset)
    guess = None if pair == "part" else gc.far_transforms(pair, offset)[1]
    o = gc.oracle(src, tgt, max_corr_dist=gate)
    e = _engine(engine_mod, src, tgt, max_corr_dist=gate)
    T_ref, info = o.align(guess=guess)
    T_gpu = e.align(guess=guess)
    d = np.abs(_moved_points(T_gpu, src) - _moved_points(T_ref, src)).max()
    print(f"{pair} {offset}: iterations {e.last_result['iterations']} / {info['iterations']}, converged "
          f"{e.hasConverged()} / {info['converged']}, max point difference {d:.3e} m")
    assert e.hasConverged() == bool(info["converged"])
    assert e.last_result["iterations"] == info["iterations"]
    assert d <= FROB_TOL
    e.close()


# ========================================== family 2: queries far larger than the target's maxabs
@pytest.mark.parametrize("dist", gc.FAR_QUERY_DIST)
def test_far_queries(engine_mod, dist):
    from oracle import ref

    tgt = gc.centred_patch()
    src = gc.far_query_source(dist)
    o = gc.oracle(src, tgt, max_corr_dist=5.0)
    e = _engine(engine_mod, src, tgt, max_corr_dist=5.0)
    _check_fitness(o, e, I4, what=f"{dist} m")
    m, _, _ = _check_sweep(o, e, I4, what=f"{dist} m gated")
    assert m == (len(src) if dist < 5.0 else 0)
    _check_sweep(o, e, gc.translation(gc.SHIFT), seeded=True, what=f"{dist} m gated seeded")
    # thresholds on both sides of the true squared distances: all kept, about half, none
    d2 = gc.nearest_d2_bruteforce(src, tgt).astype(np.float64)
    for thr, want in ((0.5 * d2.min(), "all"), (float(np.median(d2)), "some"), (2.0 * d2.max(), "none")):
        keep_ref, cnt_ref = ref.segment_differences(src, tgt, thr)
        keep, cnt = e.segment_differences(src, tgt, thr)
        np.testing.assert_array_equal(keep, keep_ref)
        assert cnt == cnt_ref
        assert {"all": cnt_ref == len(src), "some": 0 < cnt_ref < len(src), "none": cnt_ref == 0}[want], (thr, cnt_ref)
    e.close()


# ==================================================================== family 3: large rotations
@pytest.mark.parametrize("angle", gc.ROT_ANGLES)
def test_large_rotation_sweep_objective_moments(engine_mod, angle):
    src, tgt, T = gc.rotated_pair(angle)
    o = gc.oracle(src, tgt)
    e = _engine(engine_mod, src, tgt)
    m_ref, _, _ = _check_sweep(o, e, T, what=f"angle {angle:.2f}")
    assert m_ref > len(src) // 2
    _check_moments(o, e, T, m_ref, what=f"angle {angle:.2f}")
    for i, x in enumerate(gc.rotated_states()):
        _check_fdf(o, e, x, what=f"angle {angle:.2f} state {i}")
    _check_sweep(o, e, T, seeded=True, what=f"angle {angle:.2f} seeded")
    e.close()


@pytest.mark.parametrize("angle", gc.ROT_ANGLES)
def test_large_rotation_align_from_guess(engine_mod, angle):
    src, tgt, T = gc.rotated_pair(angle)
    o = gc.oracle(src, tgt)
    e = _engine(engine_mod, src, tgt)
    T_ref, info = o.align(guess=T)
    T_gpu = e.align(guess=T)
    assert e.hasConverged() == bool(info["converged"])
    assert e.last_result["iterations"] == info["iterations"]
    assert frob(T_gpu, T_ref) <= FROB_TOL
    assert np.abs(_moved_points(T_gpu, src) - _moved_points(T_ref, src)).max() <= FROB_TOL
    e.close()


# ============================================ family 4: wave, chunk and pair boundaries
def _boundary_checks(engine_mod, src, tgt, Ttrue, what):
    Tinv = np.linalg.inv(Ttrue).astype(np.float32)
    near = Tinv.copy()
    near[:3, 3] += np.float32(4e-4)
    o = gc.oracle(src, tgt)
    e = _engine(engine_mod, src, tgt)
    m_ref, _, _ = _check_sweep(o, e, Tinv, what=what + " cold")
    assert m_ref > 0
    _check_fdf(o, e, np.zeros(6), what=what + " cold x = 0")
    m_ref, _, _ = _check_sweep(o, e, near, seeded=True, what=what + " seeded")
    _check_fdf(o, e, np.array([0.001, -0.002, 0.0005, 0.0003, -0.0002, 0.0004]), what=what + " seeded x")
    _check_moments(o, e, near, m_ref, what=what)
    _check_fitness(o, e, near, what=what)
    e.close()


@pytest.mark.parametrize("n", gc.BOUNDARY_SIZES)
def test_boundary_source_sizes(engine_mod, n):
    """the first n scan points against the first 4999 CAD points (an odd target size through the pair
    copy): tails around the 64-lane wave and the 1024-point chunk"""
    src, tgt, Ttrue = gc.boundary_pair(n)
    _boundary_checks(engine_mod, src, tgt, Ttrue, f"n = {n}")


def test_boundary_tiny_target(engine_mod):
    src, tgt, Ttrue = gc.boundary_pair(65, 21)
    o = gc.oracle(src, tgt, max_corr_dist=5.0)
    e = _engine(engine_mod, src, tgt, max_corr_dist=5.0)
    Tinv = np.linalg.inv(Ttrue).astype(np.float32)
    m_ref, _, _ = _check_sweep(o, e, Tinv, what="65 vs 21 cold")
    assert m_ref > 0
    _check_fdf(o, e, np.zeros(6), what="65 vs 21 x = 0")
    m_ref, _, _ = _check_sweep(o, e, I4, seeded=True, what="65 vs 21 seeded")
    _check_fdf(o, e, np.array([0.001, -0.002, 0.0005, 0.0003, -0.0002, 0.0004]), what="65 vs 21 x")
    _check_moments(o, e, I4, m_ref, what="65 vs 21")
    _check_fitness(o, e, I4, what="65 vs 21")
    e.close()


def test_empty_and_partly_filled_chunks(engine_mod):
    """a source whose upper half sits 0.5 m above the part: in the engine's stream order (z-major grid
    order) at least one whole 1024-point chunk is rejected and at least one is partly filled; the sweep,
    the objective and the moments over those chunks equal the oracle's"""
    src, tgt, Ttrue = gc.split_source()
    Tinv = np.linalg.inv(Ttrue).astype(np.float32)
    o = gc.oracle(src, tgt)
    e = _engine(engine_mod, src, tgt)
    m_ref, tj_ref, _ = _check_sweep(o, e, Tinv, what="split cold")
    order = e.debug_source_order(len(src))
    assert sorted(order.tolist()) == list(range(len(src)))
    per_chunk = [(tj_ref[order[c:c + gc.CHUNK_PTS]] >= 0).sum() for c in range(0, len(src), gc.CHUNK_PTS)]
    print("accepted per chunk of the stream order:", per_chunk)
    assert any(c == 0 for c in per_chunk), per_chunk
    assert any(0 < c < gc.CHUNK_PTS for c in per_chunk), per_chunk
    for i, x in enumerate(gc.FDF_STATES):
        _check_fdf(o, e, np.array(x), what=f"split state {i}")
    _check_moments(o, e, Tinv, m_ref, what="split")
    m_ref, _, _ = _check_sweep(o, e, I4, seeded=True, what="split seeded")
    _check_fdf(o, e, np.zeros(6), what="split seeded")
    _check_moments(o, e, I4, m_ref, what="split seeded")
    e.close()


# ========================================== family 5: degenerate neighbourhoods, zero extent
@pytest.mark.parametrize("k", [20, 7])
@pytest.mark.parametrize("name", ["same", "line", "diag", "mix"])
def test_degenerate_covariances_bitexact(engine_mod, name, k):
    """rank-0 (coincident points; `same` has zero extent: the grid's h = 1 branch) and rank-1
    neighbourhoods: bit for bit against the oracle, on the wave / logged path and on the per-lane path"""
    from oracle import ref

    pts = gc.degenerate_clouds()[name]
    c_ref = ref.covariances(pts, k=k)
    assert np.isfinite(c_ref).all()
    for opts in ({}, {"knn_logged": 0, "knn_wave": 0}):
        e = _engine(engine_mod, pts, pts, k=k, options=opts)
        for which in ("source", "target"):
            c = e.debug_covariances(which, len(pts))
            np.testing.assert_array_equal(c, c_ref, err_msg=f"{name} k={k} {which} {opts}")
        e.close()


def test_degenerate_sweep_and_fitness(engine_mod):
    clouds = gc.degenerate_clouds()
    mix = clouds["mix"]
    o = gc.oracle(mix, mix)
    e = _engine(engine_mod, mix, mix)
    T = gc.translation((0.003, 0.002, -0.001))
    m_ref, _, _ = _check_sweep(o, e, T, what="mix cold")
    assert m_ref == len(mix)
    _check_fdf(o, e, np.array([0.003, 0.002, -0.001, 0.0, 0.0, 0.0]), what="mix at the shift")
    _check_fdf(o, e, np.array([0.001, -0.002, 0.0005, 0.0003, -0.0002, 0.0004]), what="mix")
    _check_sweep(o, e, I4, seeded=True, what="mix seeded")
    _check_fitness(o, e, T, what="mix")
    e.close()
    same = clouds["same"]
    o = gc.oracle(same, same)
    e = _engine(engine_mod, same, same)
    assert o.fitness(I4) == 0.0 and e.fitness(I4) == 0.0
    _check_fitness(o, e, T, what="same shifted")
    m_ref, _, _ = _check_sweep(o, e, T, what="same cold")
    assert m_ref == len(same)
    e.close()


# ========================================== family 6: voids inside the target's bbox
@pytest.mark.parametrize("gate", [0.04, 5.0])
def test_void_sweeps(engine_mod, gate):
    tgt, q, groups = gc.dumbbell()
    o = gc.oracle(q, tgt, max_corr_dist=gate)
    e = _engine(engine_mod, q, tgt, max_corr_dist=gate)
    shift = gc.translation((0.004, -0.003, 0.002))
    m_ref, tj_ref, _ = _check_sweep(o, e, I4, what=f"gate {gate} cold")
    a, b = groups["ball"]
    assert (tj_ref[a:b] >= 0).all() if gate > 1.0 else (tj_ref[a:b] < 0).all()
    _check_sweep(o, e, shift, what=f"gate {gate} cold shifted")
    for i, T in enumerate((I4, shift, I4)):
        _check_sweep(o, e, T, seeded=True, what=f"gate {gate} seeded {i}")
    e.close()


def test_void_fitness_and_segment_differences(engine_mod):
    from oracle import ref

    tgt, q, _ = gc.dumbbell()
    o = gc.oracle(q, tgt)
    e = _engine(engine_mod, q, tgt)
    _check_fitness(o, e, I4, what="dumbbell")
    for thr in (0.04 ** 2, 0.6 ** 2):
        keep_ref, cnt_ref = ref.segment_differences(q, tgt, thr)
        keep, cnt = e.segment_differences(q, tgt, thr)
        np.testing.assert_array_equal(keep, keep_ref)
        assert cnt == cnt_ref and 0 < cnt_ref < len(q)
    e.close()
