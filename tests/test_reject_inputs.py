"""CPU checks of tests/reject_cases.py, the cases and NumPy reference of the pre-alignment transform's calls:
the generator is the standard's, every case is what its name says, and every decision of the reference's
RANSAC runs is firm (reject_cases' docstring derives the margins), so that test_reject_gpu.py may demand the
library's decisions to equal the reference's."""
import numpy as np
import pytest

import reject_cases as rc


def test_mt19937_check_value():
    """the standard's check: the 10000th output of the default-seeded (5489) generator is 4123659995"""
    g = rc.MT19937(5489)
    v = [g() for _ in range(10000)]
    assert v[-1] == 4123659995
    # and the first outputs of seed 12345, drawn as uniform_int<>(0, INT_MAX) draws them
    s = rc.Sampler(10)
    assert [s.rnd() for _ in range(2)] == [1996335345, 1911592690]


@pytest.mark.parametrize("name", rc.RANSAC_CASES)
def test_every_decision_of_the_reference_is_firm(name):
    c, res = rc.case(name), rc.reference(name)
    bad_inlier, bad_sample = rc.non_firm(res, c)
    assert bad_inlier == 0 and bad_sample == 0, (bad_inlier, bad_sample)
    if len(c.iq) >= 3 and c.max_iterations > 0:
        assert res.selections or res.n_good_samples == 0
        assert res.samples.log


@pytest.mark.parametrize("m", rc.CLEAN_M)
def test_clean_cases_recover_their_inliers(m):
    c, res = rc.case(f"clean_{m}"), rc.reference(f"clean_{m}")
    assert len(c.iq) == m and int((c.kind == 1).sum()) == int(0.3 * m)
    assert res.outcome == "refined" and not res.kept_all
    np.testing.assert_array_equal(res.keep, c.kind == 0)
    assert res.n_iterations >= 1 and res.n_refine_rounds >= 1
    # noise well under the threshold, mismatches well over it
    S, Q = c.src[c.iq], c.tgt[c.im]
    d2 = rc.d2_float(res.T[:3], S, Q).astype(np.float64)
    assert d2[c.kind == 0].max() < 0.05 ** 2 and (m == 3 or d2[c.kind == 1].min() > 5.0 ** 2)


def test_special_cases_are_what_they_claim():
    r = rc.reference("shrink")
    assert r.outcome == "refined" and r.final_error_threshold < 0.9 * 1.5
    r = rc.reference("near_mismatches")
    c = rc.case("near_mismatches")
    assert r.outcome == "refined" and r.n_refine_rounds == 1
    np.testing.assert_array_equal(r.keep, c.kind != 1)  # the 1.1 mismatches stay
    r = rc.reference("no_refine")
    assert r.outcome == "no refine" and r.n_refine_rounds == 0 and r.n_keep == r.n_inliers_ransac >= 3
    r = rc.reference("max_iterations_0")
    assert r.outcome == "no model" and r.kept_all and r.n_iterations == 0
    r = rc.reference("max_iterations_1")
    assert r.n_iterations == 2 and r.n_refine_rounds >= 2 and not r.kept_all  # a refine of several rounds
    for m in (0, 1, 2):
        r = rc.reference(f"m_{m}")
        assert r.outcome == "m<3" and r.kept_all and r.n_keep == m
    r = rc.reference("identical_sources")
    assert r.outcome == "no model" and r.kept_all and r.n_good_samples == 0 and len(r.samples.log) == 1000
    r = rc.reference("garbage")
    assert r.n_inliers_ransac < 3 and r.kept_all and r.n_iterations == 51
    assert np.array_equal(r.T, np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("m", (1, 3, 64, 257))
def test_score_cases_sit_on_the_threshold(m):
    src, tgt, iq, im, models, thr = rc.score_case(m, 2)
    d2 = rc.d2_float(models[0][:3], src[iq], tgt[im])
    assert d2[0] == np.float32(thr * thr) and not rc.inlier(d2[:1], thr)[0]
    if m >= 3:
        assert d2[1] == np.nextafter(np.float32(2.25), np.float32(0)) and rc.inlier(d2[1:2], thr)[0]
        assert d2[2] == np.nextafter(np.float32(2.25), np.float32(9)) and not rc.inlier(d2[2:3], thr)[0]
    counts = rc.score_reference(src, tgt, iq, im, models, thr)
    assert counts[1] == 0 and np.isnan(models[1]).any()  # the model with a NaN counts nothing
    assert len(np.unique(iq)) < m or m < 3  # indices repeat


@pytest.mark.parametrize("name", rc.O2O_CASES)
def test_one_to_one_reference(name):
    im, d, nt = rc.o2o_case(name)
    order = rc.one_to_one(im, d)
    assert (im[order] >= 0).all() and (np.diff(im[order]) > 0).all()
    assert set(im[order].tolist()) == set(im[im >= 0].tolist()) and (im < nt).all()
    for p in order:
        same = np.flatnonzero(im == im[p])
        assert d[p] == d[same].min() and p == same[d[same] == d[p]].min()
    if name.startswith("fan_"):
        assert int((im == 5).sum()) == int(name[4:])


def test_svd_cases_and_the_model_rule():
    src, tgt, iq, im = rc.svd_case("integer_rigid")
    T = rc.model_f64(rc.sums15(src[iq], tgt[im]), len(iq))
    np.testing.assert_allclose(T, np.array([[0, -1, 0, 3], [0, 0, -1, -7], [1, 0, 0, 11]], np.float64), atol=1e-12)
    src, tgt, iq, im = rc.svd_case("reflection")
    T = rc.model_f64(rc.sums15(src[iq], tgt[im]), len(iq))
    assert abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-12
