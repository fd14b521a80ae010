"""The premises of tests/param_cases.py on the CPU, with the oracle alone: every case of the table is
admissible at its recorded size, the table covers what it claims (several iteration counts, the early
stops, the run to max_iter, the empty gate), the oracle's covariances at other k and gicp_epsilon are
PCL's rule, and the NumPy restatement of the stop rule decides as the oracle does."""
import numpy as np
import pytest

import param_cases as pc


def _info(case):
    return pc.oracle_align(case)[1]


@pytest.mark.parametrize("case", list(pc.CASES))
def test_every_case_is_admissible_at_its_recorded_size(case):
    """... and at no smaller size of N_CHOICES, so the table records the first admissible one"""
    f = pc.full(case)
    n = pc.CASES[case][1]
    assert n in pc.N_CHOICES
    info = _info(case)
    assert info["rc"] == 0
    print(case, n, "iterations", info["iterations"], "deltas", pc.deltas(info["trace"], f["tf_eps"], f["rot_eps"]))
    assert pc.admissible(info, f["tf_eps"], f["rot_eps"])
    for smaller in pc.N_CHOICES[:pc.N_CHOICES.index(n)]:
        assert not pc.admissible(pc.oracle_align(case, smaller)[1], f["tf_eps"], f["rot_eps"]), smaller


def test_the_table_holds_every_case_of_the_list():
    """30 cases; at most two might have been dropped, and no k, gicp_eps or max_inner_iter row"""
    kws = [kw for kw, _ in pc.CASES.values()]
    assert len(pc.CASES) == 30 and len(pc.BFGS_CASES) == 27 and len(pc.GN_CASES) == 3
    for k in (1, 5, 7, 20, 31, 32):
        assert dict(k=k) in kws
    for eps in (1e-6, 1e-2, 1.0):
        assert dict(gicp_eps=eps) in kws
    for it in (1, 2, 5, 100):
        assert dict(max_inner_iter=it) in kws
    assert len(pc.MUST_KEEP) == 15
    assert set(pc.COV_PAIRS) == {(1, 1e-3), (5, 1e-3), (7, 1e-3), (20, 1e-3), (31, 1e-3), (32, 1e-3), (20, 1e-6),
                                 (20, 1e-2), (20, 1.0), (7, 1e-2)}
    assert pc.oracle_kw("k7_eps1e-2_inner5") == dict(k=7, gicp_epsilon=1e-2, max_inner_iterations=5)


def test_the_table_is_not_trivial():
    its = {c: _info(c)["iterations"] for c in pc.BFGS_CASES}
    print(its)
    assert len(set(its.values())) >= 4, its
    for c in ("eps1", "inner1"):
        assert (_info(c)["converged"], its[c]) == (1, 1), c
    # tf_eps = 0: the ratio is 1 / 0, the delta infinite, and only max_iter stops the loop
    i = _info("tf0_iter8")
    assert (i["converged"], i["iterations"]) == (1, pc.full("tf0_iter8")["max_iter"]) == (1, 8)
    assert all(np.isinf(d) for d in pc.deltas(i["trace"], 0.0, pc.DEFAULTS["rot_eps"]))
    # max_corr_dist = 0: PCL's strict `<` accepts nothing, the solver throws in the first iteration
    i = _info("gate0")
    assert (i["converged"], i["iterations"], i["n_corr_last"], i["n_evals"]) == (0, 0, 0, 0)
    np.testing.assert_array_equal(pc.oracle_align("gate0")[0], np.eye(4, dtype=np.float32))
    # a 5 mm gate: enough for the solver, and nearly everything rejected
    i = _info("gate5mm")
    assert 4 <= i["n_corr_last"] < 0.01 * pc.CASES["gate5mm"][1], i["n_corr_last"]
    assert _info("gate_pcl_default")["n_corr_last"] == pc.CASES["gate_pcl_default"][1]  # nothing rejected
    # max_iter = 1 reports converged with a delta above 1, as PCL does
    i = _info("iter1")
    assert (i["converged"], i["iterations"]) == (1, 1)
    assert pc.deltas(i["trace"], pc.DEFAULTS["tf_eps"], pc.DEFAULTS["rot_eps"])[0] > 1 + pc.KNIFE_EDGE
    # max_inner_iter decides something: the BFGS runs of these cases end on the cap, not on the gradient test
    assert _info("inner1")["n_evals"] < _info("inner2")["n_evals"] < _info("inner5")["n_evals"]
    assert _info("inner100")["n_evals"] == _info("defaults")["n_evals"]  # 20 was never the limit here
    np.testing.assert_array_equal(pc.oracle_align("inner100")[0], pc.oracle_align("defaults")[0])


@pytest.mark.parametrize("case", list(pc.CASES))
def test_deltas_reproduce_the_oracles_stop_decision(case):
    """the deltas of the oracle's own trace, put through PCL's rule, stop where the oracle stopped -- or,
    where the oracle left through the solver's exception (not converged), do not stop at all"""
    f = pc.full(case)
    info = _info(case)
    ds = pc.deltas(info["trace"], f["tf_eps"], f["rot_eps"])
    assert len(ds) == info["iterations"]
    if info["converged"]:
        assert pc.stops_at(ds, f["max_iter"], f["fixed_iterations"]) == info["iterations"]
    else:
        assert pc.stops_at(ds, f["max_iter"], f["fixed_iterations"]) is None
        assert info["n_corr_last"] < 4  # NotEnoughPointsException


def test_state_evaluations_are_the_functor_calls_less_the_repeats():
    """ref_state_evals: of the functor calls, those at a new state.  Never more than the calls, never fewer
    than one per BFGS run, and fewer than the calls wherever a line search asked for df after f."""
    for c in pc.BFGS_CASES:
        i = _info(c)
        assert i["iterations"] <= i["n_state_evals"] <= i["n_evals"], c
        if i["iterations"]:
            assert i["n_state_evals"] < i["n_evals"], c


@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("eps", [1e-6, 1e-2, 1.0])
def test_oracle_covariances_are_pcls_rule_at_any_k_and_epsilon(k, eps):
    """ref.covariances(xyz, k, eps) against the rule restated in NumPy (param_cases.np_covariances: float
    kNN, PCL's float products summed in doubles, an fp64 SVD, singular values (1, 1, eps)) on 300 points,
    to the bar of test_oracle.py's covariance check: 1e-9 of the largest entry (measured: 1e-14)."""
    from oracle import ref

    pts = pc.clouds(2000)[1][:300]
    c_ref = ref.covariances(pts, k=k, eps=eps)
    c_np = pc.np_covariances(pts, k, eps)
    scale = np.abs(c_np).max()
    err = np.abs(c_ref - c_np).max()
    print(f"k {k} eps {eps}: max error {err:.3e}, scale {scale:.3e}")
    assert err <= 1e-9 * scale
    if eps != 1.0:
        assert np.abs(c_ref - ref.covariances(pts, k=k, eps=1.0)).max() > 1e-3  # eps reaches the result
    else:  # (1, 1, 1): the identity whatever the neighbours
        np.testing.assert_allclose(c_ref, np.tile([1.0, 0, 0, 1.0, 0, 1.0], (300, 1)), atol=1e-12)
