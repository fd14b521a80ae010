"""Objective passes skipped because the BFGS run had already passed over their fp32 transform (debug option
"pass_memo", csrc/pass_memo.hpp): the premise on a live server, and whole aligns with the table against
aligns without it, bit for bit.

Counts observed on the engine (MI355X, default parameters, scan_vs_cad(n, n); the same on the default
server, a two-block server and launched passes, as they must be -- the sums are bitwise the same):

    n        iterations   passes without   passes with   hits
    5 000    4            160              137           23
    20 000   3            71               71            0
    50 000   3            114              100           14

(the CPU oracle's default summation order shows the same 23, 0 and 14 repeats at these sizes; no size had to
be replaced by a neighbour).
"""
import functools

import numpy as np
import pytest

import pass_server_cases as pc

pytestmark = pytest.mark.gpu

_OF_THE_TEST = []


@pytest.fixture(autouse=True)
def _close_the_tests_engines():
    """a context that ran a server holds the device's one server slot until it is drained or destroyed"""
    yield
    while _OF_THE_TEST:
        _OF_THE_TEST.pop().close()


@functools.lru_cache(maxsize=None)
def _clouds(n):
    from leica_point_cloud_processing_amd import synth

    scan, cad, Ttrue = synth.scan_vs_cad(n, n)
    for a in (scan, cad, Ttrue):
        a.setflags(write=False)
    return scan, cad, Ttrue


def _engine(n, **opts):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    scan, cad, _ = _clouds(n)
    e = GICPEngine(options=opts)
    _OF_THE_TEST.append(e)
    e.set_source_xyz(scan)
    e.set_target_xyz(cad)
    return e


# ------------------------------------------------------------------------------ the premise
def test_equal_transforms_give_equal_sums_on_a_live_server():
    """Two states whose doubles differ but whose fp32 transform is the same 12 floats, alternated on ONE
    live server (mgicp_debug_fdf_sums_run runs every pass it is asked for, table or not): the four rows of
    sums are bitwise equal -- both parities of the row buffers, a one-block server whose waves hold register,
    LDS and streamed chunks."""
    from oracle import ref

    n = 50000
    m = pc.server_model(n, 1)
    assert m.servable and m.reg_chunks and m.lds_chunks and m.streamed_chunks, m
    x = np.array(pc.X_SMALL, np.float64)
    x2 = x * (1.0 + 2.0 ** -40)  # far below half an ulp of the fp32 values the transform is built from
    assert not np.any(x == x2)
    A, A2 = ref.apply_state(x), ref.apply_state(x2)
    assert np.array_equal(A[:3].view(np.uint32), A2[:3].view(np.uint32))
    e = _engine(n, srv_cus=1)
    cnt, _, _ = e.debug_correspondences(pc.sweep_transform(_clouds(n)[2]), n)
    assert cnt > n // 2, cnt
    before = e.pass_stats()
    got = e.debug_fdf_sums_run(np.array([x, x2, x, x2]))
    after = e.pass_stats()
    d = {k: after[k] - before[k] for k in after}
    assert (d["server_launches"], d["server_passes"], d["launched_passes"], d["takeovers"], d["memo_hits"]) == \
        (1, 4, 0, 0, 0), d
    assert got[0, 13] == cnt
    for k in range(1, 4):
        np.testing.assert_array_equal(got[k].view(np.uint64), got[0].view(np.uint64), err_msg=f"pass {k}")


# ------------------------------------------------------------------------------ whole aligns
FORMS = {"server": {}, "small_server": {"srv_cus": 2}, "launched": {"resident": 0}}
# sizes at which a run of the engine repeats a transform; 20 000 is the control (the oracle repeats none)
WITH_HITS = (5000, 50000)


def _align(e):
    before = e.pass_stats()
    T = e.align()
    r = e.last_result
    after = e.pass_stats()
    passes = (after["server_passes"] + after["launched_passes"] - after["takeovers"]) - \
        (before["server_passes"] + before["launched_passes"] - before["takeovers"])
    assert passes == r["n_evals"], (passes, r["n_evals"])  # n_evals keeps meaning "device passes run"
    return dict(T=T.copy(), iterations=r["iterations"], n_corr=r["n_corr"], n_evals=r["n_evals"],
                converged=r["converged"], hits=after["memo_hits"] - before["memo_hits"],
                trace=[np.asarray(t, np.float32) for t in e.debug_trace(200)])


def _same(a, b, what):
    np.testing.assert_array_equal(a["T"].view(np.uint32), b["T"].view(np.uint32), err_msg=what)
    assert (a["iterations"], a["n_corr"], a["converged"]) == (b["iterations"], b["n_corr"], b["converged"]), what
    assert len(a["trace"]) == len(b["trace"]) == a["iterations"], what
    for u, v in zip(a["trace"], b["trace"]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32), err_msg=what)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [5000, 20000, 50000])
def test_aligns_with_the_table_equal_aligns_without(n, form):
    """T, iterations, n_corr and every per-iteration transform of an align with "pass_memo" 1 are bitwise
    those of "pass_memo" 0; every pass the table saved is a hit: n_evals(0) == n_evals(1) + hits(1).

    The aligns here have several outer iterations, each a BFGS run of its own over new correspondences,
    and run k + 1 starts at the transform run k ended on: a table that outlived its run would answer that
    first evaluation with the previous correspondences' sums and the trace would differ.  The table
    belongs to the run's functor, not to the context.

    A second align on the same context repeats the first (T, n_evals, hits): nothing of the table is left
    from one align to the next."""
    on = _engine(n, pass_memo=1, **FORMS[form])
    a = _align(on)
    a2 = _align(on)
    on.close()
    off = _engine(n, pass_memo=0, **FORMS[form])
    b = _align(off)
    off.close()
    print(f"n {n} {form}: iterations {a['iterations']}, passes without {b['n_evals']}, with {a['n_evals']}, "
          f"hits {a['hits']}")
    assert a["iterations"] > 1, a["iterations"]  # more than one BFGS run: the table's scope is exercised
    _same(a, b, "pass_memo 1 against pass_memo 0")
    assert b["hits"] == 0
    assert b["n_evals"] == a["n_evals"] + a["hits"], (b["n_evals"], a["n_evals"], a["hits"])
    if n in WITH_HITS:
        assert a["hits"] > 0 and a["n_evals"] < b["n_evals"]
    _same(a2, a, "second align on the context")
    assert (a2["n_evals"], a2["hits"]) == (a["n_evals"], a["hits"])


def test_counts_do_not_depend_on_the_pass_path():
    """every form of the engine hits and misses on the same evaluations (the sums are bitwise the same)"""
    n = 5000
    got = {}
    for form, opts in FORMS.items():
        e = _engine(n, **opts)
        a = _align(e)
        e.close()
        got[form] = (a["iterations"], a["n_evals"], a["hits"])
    assert len(set(got.values())) == 1, got
