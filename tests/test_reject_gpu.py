"""mgicp_reject_ransac, mgicp_reject_one_to_one and mgicp_estimate_rigid_svd (the pre-alignment transform:
InitialAlignment::rejectCorrespondences, rejectOneToOneCorrespondences, estimateTransform) on the GPU against
the NumPy reference of tests/reject_cases.py.

The scoring kernel and the one-to-one rejector are compared bit for bit.  The RANSAC run's decisions --
keep, the counts, the loop's and the refine's lengths -- must equal the reference's, which
test_reject_inputs.py shows to be firm; the models may differ by one float ulp per entry (fixed-tree sums and
a Jacobi against fsum and LAPACK).  The 15 sums are held to the standard bound of a recursive sum.
"""
import ctypes

import numpy as np
import pytest

import reject_cases as rc

pytestmark = pytest.mark.gpu

_ENGINE = []
_RUNS = {}


def _engine():
    from leica_point_cloud_processing_amd.engine import GICPEngine

    if not _ENGINE:
        _ENGINE.append(GICPEngine())
    return _ENGINE[0]


def _ransac(e, c):
    return e.reject_ransac(c.src, c.tgt, c.iq, c.im, c.threshold, c.max_iterations, c.refine)


def _run(name):
    """the engine's outputs for a RANSAC case, computed once and shared: (keep, T, info)"""
    if name not in _RUNS:
        _RUNS[name] = _ransac(_engine(), rc.case(name))
    return _RUNS[name]


def _ulps(got, want):
    """the distance of got from want in units of want's float32 spacing"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _records(xyz, stride):
    """the points in records of `stride` bytes, the floats between them NaN"""
    rec = np.full((max(len(xyz), 1), stride // 4), np.nan, np.float32)
    rec[:len(xyz), :3] = xyz
    return rec[:len(xyz)] if len(xyz) else rec[:0]


# ---- scoring: bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 2, 3, 63, 64, 65, 255, 256, 257, 4099))
def test_scoring_equals_the_float32_reference_exactly(m):
    e = _engine()
    for n_models in (1, 2, 63, 64):
        src, tgt, iq, im, models, thr = rc.score_case(m, n_models)
        want = rc.score_reference(src, tgt, iq, im, models, thr)
        got = e.debug_score_models(src, tgt, iq, im, models, thr)
        np.testing.assert_array_equal(got, want, err_msg=f"B = {n_models}")
        if n_models > 1:
            assert got[n_models // 2] == 0  # the model with a NaN
    # the three correspondences on the threshold, under the identity: only the one a float step inside counts
    if m >= 3:
        src, tgt, iq, im, models, thr = rc.score_case(m, 1)
        assert e.debug_score_models(src, tgt, iq[:3], im[:3], models, thr)[0] == 1
        assert e.debug_score_models(src, tgt, iq[:1], im[:1], models, thr)[0] == 0


@pytest.mark.parametrize("strides", ((12, 16), (16, 32), (32, 12), (32, 32)))
def test_scoring_reads_strided_records(strides):
    e = _engine()
    src, tgt, iq, im, models, thr = rc.score_case(257, 5)
    want = rc.score_reference(src, tgt, iq, im, models, thr)
    got = e.debug_score_models(_records(src, strides[0]), _records(tgt, strides[1]), iq, im, models, thr)
    np.testing.assert_array_equal(got, want)
    # more models than one launch holds, and one launch per model
    src, tgt, iq, im, models, thr = rc.score_case(300, 64, seed=1)
    many = np.concatenate([models, models[::-1], models[:7]])
    want = rc.score_reference(src, tgt, iq, im, many, thr)
    np.testing.assert_array_equal(e.debug_score_models(src, tgt, iq, im, many, thr), want)
    e.debug_option("ransac_batch", 1)
    try:
        np.testing.assert_array_equal(e.debug_score_models(src, tgt, iq, im, many[:9], thr), want[:9])
    finally:
        e.debug_option("ransac_batch", 0)


# ---- RANSAC ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.RANSAC_CASES)
def test_ransac_equals_the_reference(name):
    c, ref = rc.case(name), rc.reference(name)
    keep, T, info = _run(name)
    print(name, ref.outcome, {k: info[k] for k in ("n_hypotheses", "n_iterations", "n_refine_rounds",
                                                   "n_inliers_ransac", "n_inliers_final", "n_keep",
                                                   "final_error_threshold", "ms_device")})
    np.testing.assert_array_equal(keep, ref.keep)
    assert info["n_keep"] == ref.n_keep
    assert info["n_iterations"] == ref.n_iterations and info["n_skipped"] == 0
    assert info["n_inliers_ransac"] == ref.n_inliers_ransac
    assert info["n_refine_rounds"] == ref.n_refine_rounds
    if ref.kept_all:
        np.testing.assert_array_equal(T, np.eye(4, dtype=np.float32))
        assert keep.all()
    else:
        worst = _ulps(T[:3], ref.T[:3]).max()
        print("  worst entry of best_T:", worst, "ulp")
        assert worst <= 1.0
        np.testing.assert_array_equal(T[3], [0, 0, 0, 1])
        assert info["n_inliers_final"] == ref.n_keep
    # the refine's last threshold: a square root of a float's multiple, or the caller's value itself
    assert abs(info["final_error_threshold"] - ref.final_error_threshold) <= 1e-3 * ref.final_error_threshold
    m = len(c.iq)
    assert info["pair_tests"] >= m * ref.n_iterations and info["n_hypotheses"] >= ref.n_iterations


@pytest.mark.parametrize("name", ("clean_65", "clean_4099", "shrink", "max_iterations_1", "no_refine", "garbage"))
def test_ransac_does_not_depend_on_the_batch_or_the_call(name):
    c = rc.case(name)
    keep, T, info = _run(name)
    e = _engine()
    again = _ransac(e, c)
    e.debug_option("ransac_batch", 1)
    try:
        one = _ransac(e, c)
    finally:
        e.debug_option("ransac_batch", 0)
    seven = None
    e.debug_option("ransac_batch", 7)
    try:
        seven = _ransac(e, c)
    finally:
        e.debug_option("ransac_batch", 0)
    for other in (again, one, seven):
        assert other[0].tobytes() == keep.tobytes() and other[1].tobytes() == T.tobytes()
        for f in ("n_iterations", "n_refine_rounds", "n_inliers_ransac", "n_inliers_final", "final_error_threshold",
                  "n_keep"):
            assert other[2][f] == info[f], f
    assert one[2]["n_hypotheses"] == info["n_iterations"] or info["n_iterations"] == 0


def test_ransac_reads_strided_records_and_refuses_bad_arguments():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    c = rc.case("clean_65")
    keep, T, _info = _run("clean_65")
    got = e.reject_ransac(_records(c.src, 32), _records(c.tgt, 16), c.iq, c.im, c.threshold, c.max_iterations, True)
    assert got[0].tobytes() == keep.tobytes() and got[1].tobytes() == T.tobytes()
    bad = c.im.copy()
    bad[5] = len(c.tgt)
    for args in ((c.src, c.tgt, c.iq, bad, 1.5, 1000), (c.src, c.tgt, -c.iq - 1, c.im, 1.5, 1000),
                 (c.src, c.tgt, c.iq, c.im, -1.0, 1000), (c.src, c.tgt, c.iq, c.im, float("nan"), 1000),
                 (c.src, c.tgt, c.iq, c.im, 1.5, -1)):
        with pytest.raises(_lib.MgicpError) as err:
            e.reject_ransac(*args)
        assert err.value.code == _lib.MGICP_E_INVALID
    # a bad stride, through the C call itself
    k = np.zeros(len(c.iq), np.uint8)
    n = ctypes.c_size_t()
    Tb = np.zeros(16, np.float32)
    for ss, ts in ((8, 12), (12, 14)):
        rc_ = e._lib.mgicp_reject_ransac(e._h, c.src.ctypes.data, len(c.src), ss, c.tgt.ctypes.data, len(c.tgt), ts,
                                         c.iq.ctypes.data, c.im.ctypes.data, len(c.iq), 1.5, 1000, 1, k.ctypes.data,
                                         ctypes.byref(n), Tb.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None)
        assert rc_ == _lib.MGICP_E_INVALID


def test_rejectors_leave_a_set_source_and_target_alone(cube_clouds):
    """an align before and after the three calls is equal: no cloud slot, no cached state is touched"""
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, _T = cube_clouds
    c = rc.case("clean_1000")
    with GICPEngine() as e:
        e.set_source_xyz(src)
        e.set_target_xyz(tgt)
        before = e.align().copy()
        res_before = dict(e.last_result)
        keep, T, _info = _ransac(e, c)
        e.reject_one_to_one(c.im, np.ones(len(c.im), np.float32), len(c.tgt))
        e.estimate_rigid_svd(c.src, c.tgt, c.iq[keep], c.im[keep])
        e.boundary_points(c.src, np.tile(np.float32([0, 0, 1]), (len(c.src), 1)), 5, 1.0)  # fills the helper slot
        _ransac(e, c)
        after = e.align()
        assert after.tobytes() == before.tobytes()
        assert e.last_result["iterations"] == res_before["iterations"]
    ref_keep, ref_T, _i = _run("clean_1000")
    assert keep.tobytes() == ref_keep.tobytes() and T.tobytes() == ref_T.tobytes()


# ---- one-to-one: exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.O2O_CASES)
def test_one_to_one_equals_the_reference(name):
    e = _engine()
    im, d, nt = rc.o2o_case(name)
    want = rc.one_to_one(im, d)
    order, info = e.reject_one_to_one(im, d, nt)
    np.testing.assert_array_equal(order, want)
    assert info["n_keep"] == len(want)
    assert (np.diff(im[order]) > 0).all()  # ascending index_match, one survivor per target
    again, _ = e.reject_one_to_one(im, d, nt)
    assert again.tobytes() == order.tobytes()


def test_one_to_one_refuses_nan_negative_and_out_of_range():
    from leica_point_cloud_processing_amd import _lib

    e = _engine()
    im, d, nt = rc.o2o_case("m_64")
    for bad_d, bad_im in ((np.nan, None), (-1.0, None), (None, nt)):
        d2, im2 = d.copy(), im.copy()
        if bad_d is not None:
            d2[7] = bad_d
        if bad_im is not None:
            im2[7] = bad_im
        with pytest.raises(_lib.MgicpError) as err:
            e.reject_one_to_one(im2, d2, nt)
        assert err.value.code == _lib.MGICP_E_INVALID


# ---- the SVD estimate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("noisy_3", "noisy_64", "noisy_257", "noisy_4099"))
def test_svd_sums_and_transform(name):
    e = _engine()
    src, tgt, iq, im = rc.svd_case(name)
    m = len(iq)
    T, info = e.estimate_rigid_svd(src, tgt, iq, im)
    want = rc.sums15(src[iq], tgt[im])
    bound = (m - 1) * 2.0 ** -53 * rc.sum_terms_abs(src[iq], tgt[im])
    err = np.abs(info["sums"] - want)
    print(name, "sums: worst error / bound", float((err / bound).max()))
    assert (err <= bound).all()
    ref = rc.model(want, m)
    worst = _ulps(T[:3], ref).max()
    print(name, "T: worst entry", worst, "ulp")
    assert worst <= 1.0
    np.testing.assert_array_equal(T[3], [0, 0, 0, 1])
    T2, info2 = e.estimate_rigid_svd(_records(src, 32), _records(tgt, 16), iq, im)
    assert T2.tobytes() == T.tobytes() and info2["sums"].tobytes() == info["sums"].tobytes()


def test_svd_recovers_an_exact_rigid_motion():
    e = _engine()
    src, tgt, iq, im = rc.svd_case("integer_rigid")
    T, info = e.estimate_rigid_svd(src, tgt, iq, im)
    np.testing.assert_array_equal(info["sums"], rc.sums15(src[iq], tgt[im]))  # integers: every sum is exact
    R = T[:3, :3].astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 2.0 ** -23
    np.testing.assert_allclose(T[:3], [[0, -1, 0, 3], [0, 0, -1, -7], [1, 0, 0, 11]], atol=2.0 ** -20)


def test_svd_of_a_mirror_image_is_a_proper_rotation():
    e = _engine()
    src, tgt, iq, im = rc.svd_case("reflection")
    T, _info = e.estimate_rigid_svd(src, tgt, iq, im)
    R = T[:3, :3].astype(np.float64)
    assert abs(np.linalg.det(R) - 1.0) < 1e-6 and np.abs(R.T @ R - np.eye(3)).max() < 1e-6
    ref = rc.model(rc.sums15(src[iq], tgt[im]), len(iq))
    assert _ulps(T[:3], ref).max() <= 1.0


def test_svd_of_nothing_and_of_degenerate_sets():
    e = _engine()
    src, tgt, iq, im = rc.svd_case("noisy_64")
    T, info = e.estimate_rigid_svd(src, tgt, iq[:0], im[:0])
    np.testing.assert_array_equal(T, np.eye(4, dtype=np.float32))
    assert not info["sums"].any()
    for m in (1, 2):  # rank-deficient: some proper rotation that maps the means onto each other
        T, _ = e.estimate_rigid_svd(src, tgt, iq[:m], im[:m])
        R = T[:3, :3].astype(np.float64)
        assert abs(np.linalg.det(R) - 1.0) < 1e-5 and np.abs(R.T @ R - np.eye(3)).max() < 1e-5
        sm, tm = src[iq[:m]].astype(np.float64).mean(0), tgt[im[:m]].astype(np.float64).mean(0)
        np.testing.assert_allclose(R @ sm + T[:3, 3], tm, atol=1e-4)


# ---- the chain ------------------------------------------------------------------------------------------
def test_run_keypoints_based_algorithm_equals_its_members():
    import boundary_cases as bc
    from leica_point_cloud_processing_amd import initial_alignment as ia

    e = _engine()
    xyz, nrm, _k = bc.case("part")
    a = 0.2
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    xyz_t = (xyz.astype(np.float64) @ R.T + [0.05, -0.02, 0.01]).astype(np.float32)
    nrm_t = (nrm.astype(np.float64) @ R.T).astype(np.float32)
    T, exists, steps = ia.runKeypointsBasedAlgorithm((xyz, nrm), (xyz_t, nrm_t), "BOUNDARY", engine=e)
    assert exists and T.shape == (4, 4)
    # the members, one by one
    _s, skp, _n = ia.obtainBoundaryKeypoints(xyz, nrm, e)
    _s, tkp, _n = ia.obtainBoundaryKeypoints(xyz_t, nrm_t, e)
    _s, sf = ia.obtainFeatures(xyz, nrm, skp, engine=e)
    _s, tf = ia.obtainFeatures(xyz_t, nrm_t, tkp, engine=e)
    sk, tk = xyz[skp], xyz_t[tkp]
    corr = ia.obtainCorrespondences(sf, tf, e)
    assert len(corr[0]) > 10
    corr1 = ia.rejectCorrespondences(sk, tk, corr, e)
    for got, want in zip(steps["correspondences_ransac"], corr1):
        assert np.asarray(got).tobytes() == np.asarray(want).tobytes()
    one = len(corr1[0]) > len(xyz) // 2
    assert steps["one_to_one"] == one
    corr2 = ia.rejectOneToOneCorrespondences(corr1, len(tk), e) if one else corr1
    for got, want in zip(steps["correspondences_final"], corr2):
        assert np.asarray(got).tobytes() == np.asarray(want).tobytes()
    T1, exists1 = ia.estimateTransform(sk, tk, corr2, e)
    assert exists1 and T1.tobytes() == T.tobytes()
    # the one-to-one member on what the chain found, whatever the size rule said: one survivor per target,
    # the nearest, in ascending index_match
    q, mt, d = ia.rejectOneToOneCorrespondences(corr1, len(tk), e)
    np.testing.assert_array_equal(q, corr1[0][rc.one_to_one(corr1[1], corr1[2])])
    assert (np.diff(mt) > 0).all() and len(d) == len(q)
