"""CPU certification of tests/harris_cases.py: every cloud is what it claims to be and the rules the GPU
tests (tests/test_harris_gpu.py) lean on hold for the NumPy reference alone.  No engine here."""
import numpy as np
import pytest

import harris_cases as hc
import normals_cases as nc


def _keypoints(name, response=None):
    xyz, nrm, radius, thr, nonmax = hc.case(name)
    ref = hc.case_reference(name)
    return hc.keypoint_rule(ref, ref.response if response is None else response, thr, nonmax)


@pytest.mark.parametrize("name", hc.NMS_CASES)
def test_suppression_cases_hold_suppressed_candidates_and_keypoints(name):
    kp, cand, _tied = _keypoints(name)
    assert len(kp) > 0, "no keypoint: the case would show nothing"
    assert cand.sum() > len(kp), "no suppressed candidate: the second sweep would show nothing"
    assert cand[kp].all() and (np.diff(kp) > 0).all()


def test_regimes_of_the_scans():
    """1.4 resolutions is the reference's regime: 1-10 neighbours, a mean near 2.5, tens of candidates; at 3
    and 10 resolutions most records are candidates and the suppression does the work"""
    for which in ("cube", "part"):
        stats = []
        for tag in ("1p4", "3", "10"):
            ref = hc.case_reference(f"{which}_{tag}")
            kp, cand, _t = _keypoints(f"{which}_{tag}")
            stats.append((ref.count[ref.finite].mean(), int(ref.count.max()), int(cand.sum()), len(kp)))
        assert 2.0 < stats[0][0] < 3.0 and stats[0][1] <= 10 and 10 <= stats[0][2] <= 100
        assert stats[0][2] < stats[1][2] < stats[2][2] and stats[2][2] > 0.7 * hc.case_reference(f"{which}_10").n
        assert stats[2][0] > 64          # sets larger than a wave
        assert all(0 < s[3] < s[2] for s in stats)


def test_ties_are_present():
    """the `0.04f +` quantises the response: neighbours with equal responses exist, and both stay"""
    for name in ("cube_3", "part_1p4", "nonfinite", "far_part"):
        _kp, _cand, tied = _keypoints(name)
        assert tied.sum() > 0, name
    for name in ("dups", "flat"):
        kp, _cand, tied = _keypoints(name)
        assert len(kp) > 0 and tied[kp].all(), name


@pytest.mark.parametrize("name", hc.CASES)
def test_share_of_non_firm_covar_entries(name):
    ref = hc.case_reference(name)
    assert hc.nonfirm_share(ref) <= hc.NONFIRM_CAP
    assert np.isfinite(ref.e).all() and (ref.e >= 0).all()


def test_midpoint_distance_alone_would_not_decide_small_sets():
    """why harris_cases counts an entry computed without any rounding as firm: at 1.4 resolutions the mean
    of two or four float products lands exactly on a float32 midpoint in a large share of the entries"""
    for name in ("cube_1p4", "part_1p4"):
        ref = hc.case_reference(name)
        with np.errstate(invalid="ignore"):
            lo = np.nextafter(ref.covar, np.float32(-np.inf)).astype(np.float64)
            hi = np.nextafter(ref.covar, np.float32(np.inf)).astype(np.float64)
            c64 = ref.covar.astype(np.float64)
            on_mid = (ref.exact == (c64 + lo) / 2) | (ref.exact == (c64 + hi) / 2)
        rows = ref.finite
        share = on_mid[rows].sum() / (6.0 * rows.sum())
        assert share > 5 * hc.NONFIRM_CAP, share
        assert ref.no_rounding[on_mid & rows[:, None]].all()


def test_lattice_rim_set_sizes_against_integers():
    from scipy.spatial import cKDTree

    xyz, _nrm, radius, _thr, _nm = hc.case("lattice_rim")
    ref = hc.case_reference("lattice_rim")
    ij = nc.lattice_rim_ij()
    assert radius == 5 * nc.LATTICE_RIM_STEP and len(ij) == len(xyz)
    # integer d2 < 25 <=> d2 <= 24: any radius strictly between sqrt(24) and 5
    sets = cKDTree(ij.astype(np.float64)).query_ball_point(ij.astype(np.float64), 4.95)
    want = np.array([len(s) for s in sets])
    np.testing.assert_array_equal(ref.count, want)
    d2 = ((ij[:600, None, :] - ij[None, :, :]) ** 2).sum(-1)
    assert (d2 == 25).sum() > 100 and (d2 == 24).sum() > 100        # pairs on the rim and one step inside


def test_response_model_orders_like_fp64_on_firm_records():
    """the float32 model of the response (what the GPU test holds the engine's response to) agrees with
    the fp64 evaluation of the same expression to within its rounding, and orders set pairs the same way
    wherever fp64 separates them by more than that"""
    for name in hc.CLOUD_CASES:
        ref = hc.case_reference(name)
        r64, mag = hc.response_fp64(ref.covar)
        ok = ref.finite & ref.firm.all(1) & np.isfinite(r64)
        bound = 16 * 2.0 ** -24 * mag                     # 14 float operations, each within 2^-24 of a partial
        err = np.abs(ref.response.astype(np.float64) - r64)
        assert (err[ok] <= bound[ok]).all(), name
        gi, gj = ref.fin_idx[ref.I], ref.fin_idx[ref.J]
        sel = ok[gi] & ok[gj]
        gi, gj = gi[sel], gj[sel]
        clear = np.abs(r64[gi] - r64[gj]) > bound[gi] + bound[gj]
        lt32 = ref.response[gi] < ref.response[gj]
        lt64 = r64[gi] < r64[gj]
        assert clear.sum() > 0 or len(gi) == 0 or name == "flat", name
        np.testing.assert_array_equal(lt32[clear], lt64[clear], err_msg=name)


def test_clump_reaches_the_hand_off_in_both_sweeps():
    """a cell box contains its record's set, so a set above kHarLaneCap is a box above it: such records
    leave the lane kernels -- in the response sweep all of them, in the suppression sweep the candidates
    among them, suppressed ones and a keypoint alike; the sheet's records stay with the lanes' walk"""
    ref = hc.case_reference("clump")
    kp, cand, _t = _keypoints("clump")
    big = ref.count > hc.LANE_CAP
    assert big.sum() > 500 and (cand & big).sum() > 500
    assert big[kp].any() and (cand & big).sum() > big[kp].sum()
    assert (ref.count == 1).sum() >= 1500           # the sheet


def test_nonfinite_case_claims():
    xyz, nrm, _radius, thr, _nm = hc.case("nonfinite")
    ref = hc.case_reference("nonfinite")
    kp, cand, _t = _keypoints("nonfinite")
    assert (~ref.finite).sum() == 50
    lone = np.array(hc.NONFINITE_LONE)
    assert (ref.count[lone] == 3).all() and (ref.c[lone] == 0).all()
    assert (ref.covar[lone] == 0).all() and (ref.response[lone] == 0).all() and not cand[lone].any()
    nan_x = np.isnan(nrm[:, 0]) & ref.finite
    nan_y = np.isfinite(nrm[:, 0]) & np.isnan(nrm[:, 1]) & ref.finite
    inf_z = np.isinf(nrm[:, 2]) & np.isfinite(nrm[:, 0]) & ref.finite
    assert nan_x.sum() >= 20 and nan_y.sum() == 20 and inf_z.sum() == 10
    # a NaN x is not counted; a NaN y or an infinite z goes through the sums
    assert (ref.c < ref.count).sum() > 20 and (ref.c[nan_y] == ref.count[nan_y]).all()
    bad = ~np.isfinite(ref.response)
    assert bad[nan_y].all() and bad[inf_z].all() and bad.sum() > 100 and not cand[bad].any()
    # a keypoint with a NaN response in its set: the NaN suppressed nothing
    gi, gj = ref.fin_idx[ref.I], ref.fin_idx[ref.J]
    iskp = np.zeros(ref.n, bool)
    iskp[kp] = True
    assert (iskp[gi] & np.isnan(ref.response[gj])).any()


def test_dups_and_flat_claims():
    xyz, _nrm, _r, _thr, _nm = hc.case("dups")
    ref = hc.case_reference("dups")
    kp, _cand, _t = _keypoints("dups")
    _u, inv, cnt = np.unique(xyz, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    assert (cnt == 3).all()
    order = np.argsort(inv, kind="stable").reshape(-1, 3)
    for col in (1, 2):
        np.testing.assert_array_equal(ref.covar[order[:, 0]].view(np.uint32), ref.covar[order[:, col]].view(np.uint32))
    iskp = np.zeros(ref.n, bool)
    iskp[kp] = True
    assert (iskp[order].sum(1) % 3 == 0).all() and len(kp) % 3 == 0      # a copy brings its twins
    ref = hc.case_reference("flat")
    kp, cand, tied = _keypoints("flat")
    fin = ref.finite
    assert len(np.unique(ref.covar[fin].view(np.uint32), axis=0)) == 1 and ref.no_rounding[fin].all()
    np.testing.assert_array_equal(kp, np.flatnonzero(fin))
    assert (ref.count[fin] >= 2).all()


def test_edge_value_cases():
    ref = hc.case_reference("radius_zero")
    kp, cand, _t = _keypoints("radius_zero")
    assert (ref.count == 0).all() and (ref.response == 0).all() and len(kp) == 0 and not cand.any()
    kp, _c, _t = hc.keypoint_rule(ref, ref.response, np.float32(0.0))
    assert len(kp) == ref.n                      # a threshold of 0 keeps the zero responses
    assert hc.case_reference("n0").n == 0 and len(_keypoints("n0")[0]) == 0
    ref = hc.case_reference("n1")
    assert ref.count.tolist() == [1] and _keypoints("n1")[0].tolist() == [0]
    kp, _cand, tied = _keypoints("part_all")
    np.testing.assert_array_equal(kp, np.arange(6000))
    assert not tied.any()
