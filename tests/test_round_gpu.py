"""r08, the steady-state round (DESIGN.md "r08: the steady-state round"): a fused listed sweep whose counters
come back zero ends its round at the query kernel (debug option "round_fast"), and a single rank's host takes
the row total while the rows land ("rows_running").  Every test compares against the same engine in its form
before r08 -- "round_fast" 0, "rows_running" 0 -- bit for bit: T, the per-iteration trace, iterations, n_corr,
and where a test takes sweeps through mgicp_debug_correspondences, their indices and Mahalanobis matrices.
mgicp_debug_round_stats says which path each round took.

Observed (MI355X, scan_vs_cad(20 000, 20 000), 3 outer iterations per align): aligns 1-2 three slow rounds
each (cold sweeps), aligns 3-4 three slow rounds each, all with pending queries and deferred chunks, aligns
5-6 three fast rounds each.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OLD = {"round_fast": 0, "rows_running": 0}
N = 20000

_OF_THE_TEST = []


@pytest.fixture(autouse=True)
def _close_the_tests_engines():
    """a context that ran a server holds the device's one server slot until it is drained or destroyed"""
    yield
    while _OF_THE_TEST:
        _OF_THE_TEST.pop().close()


@functools.lru_cache(maxsize=None)
def _clouds(n_scan, n_cad, clutter=0.0, debris=0):
    from leica_point_cloud_processing_amd import synth

    scan, cad, Ttrue = synth.scan_vs_cad(n_scan, n_cad, clutter=clutter, debris=debris)
    for a in (scan, cad, Ttrue):
        a.setflags(write=False)
    return scan, cad, Ttrue


def _engine(scan, cad, options=None, **params):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    e = GICPEngine(options=options or {}, **params)
    _OF_THE_TEST.append(e)
    e.set_source_xyz(scan)
    e.set_target_xyz(cad)
    return e


def _align(e):
    """one align: its result and the rounds / passes it took"""
    r0, p0 = e.round_stats(), e.pass_stats()
    T = e.align()
    r = e.last_result
    r1, p1 = e.round_stats(), e.pass_stats()
    return dict(T=T.copy(), iterations=r["iterations"], n_corr=r["n_corr"], converged=e.hasConverged(),
                n_evals=r["n_evals"], trace=[np.asarray(t, np.float32) for t in e.debug_trace(200)],
                rounds={k: r1[k] - r0[k] for k in r1}, passes={k: p1[k] - p0[k] for k in p1})


def _same(a, b, what):
    np.testing.assert_array_equal(a["T"].view(np.uint32), b["T"].view(np.uint32), err_msg=what)
    assert (a["iterations"], a["n_corr"], a["converged"], a["n_evals"]) == \
        (b["iterations"], b["n_corr"], b["converged"], b["n_evals"]), what
    assert len(a["trace"]) == len(b["trace"]), what
    for u, v in zip(a["trace"], b["trace"]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32), err_msg=what)


def _same_sweep(a, b, what):
    (ma, ta, Ma), (mb, tb, Mb) = a, b
    assert ma == mb, what
    np.testing.assert_array_equal(ta, tb, err_msg=what)
    np.testing.assert_array_equal(Ma.view(np.uint64), Mb.view(np.uint64), err_msg=what)


def _rounds(a):
    return a["rounds"]["fast"] + a["rounds"]["slow"]


# ------------------------------------------------------------------------------ steady state
def test_steady_state_rounds_are_fast_and_aligns_equal():
    """Six aligns of one cloud pair: 1-2 run the cold sweep, 3-4 build the lists (pending queries, build
    requests: slow rounds), 5-6 find every queried cell listed and every accepted point's covariance
    computed: only fast rounds.  The form before r08 reports no fast round and gives the same aligns."""
    scan, cad, Ttrue = _clouds(N, N)
    new, old = _engine(scan, cad), _engine(scan, cad, OLD)
    got = []
    for k in range(6):
        a, b = _align(new), _align(old)
        print(f"align {k + 1}: iterations {a['iterations']}, rounds {a['rounds']} | before r08 {b['rounds']}")
        _same(a, b, f"align {k + 1}")
        assert a["iterations"] > 1
        assert _rounds(a) == _rounds(b) == a["iterations"]  # one round per outer iteration
        assert b["rounds"]["fast"] == 0
        got.append(a)
    for k in (0, 1):  # cold sweeps: not listed, never fast
        assert got[k]["rounds"]["fast"] == 0, got[k]["rounds"]
    for k in (2, 3):
        assert got[k]["rounds"]["slow"] > 0 and got[k]["rounds"]["pending"] > 0, (k, got[k]["rounds"])
    for k in (4, 5):
        assert got[k]["rounds"] == {"fast": got[k]["iterations"], "slow": 0, "deferred": 0, "pending": 0}, got[k]["rounds"]
        assert got[k]["passes"]["takeovers"] == 0 and got[k]["passes"]["launched_passes"] == 0, got[k]["passes"]
    # sweeps at new transforms over the built lists: listed cells and new ones mixed
    I = np.eye(4, dtype=np.float32)
    off = np.eye(4, dtype=np.float32)
    off[:3, 3] = [0.004, -0.003, 0.02]
    Tinv = np.linalg.inv(Ttrue).astype(np.float32)
    for j, T in enumerate([Tinv, Tinv, off, Tinv, off, I]):
        _same_sweep(new.debug_correspondences(T, N), old.debug_correspondences(T, N), f"sweep {j}")
    _same(_align(new), _align(old), "align after the sweeps")


def test_lists_from_the_first_sweep_with_lazy_covariances():
    """"vlist_cold" 0, synchronous lazy source mode, a scan with clutter and debris: the first listed sweep
    finds no list (every query pending) and, once answered, accepts points without a covariance: slow rounds
    with deferred chunks.  Later aligns find lists and covariances in place: fast rounds only."""
    scan, cad, _ = _clouds(N, N, clutter=0.04, debris=400)
    opts = {"vlist_cold": 0, "async_cov": 0, "lazy_src_cov": 1}
    new, old = _engine(scan, cad, opts), _engine(scan, cad, {**opts, **OLD})
    got = []
    for k in range(5):
        a, b = _align(new), _align(old)
        print(f"align {k + 1}: iterations {a['iterations']}, rounds {a['rounds']}")
        _same(a, b, f"align {k + 1}")
        got.append(a)
    assert got[0]["rounds"]["slow"] > 0 and got[0]["rounds"]["deferred"] > 0, got[0]["rounds"]
    assert got[-1]["rounds"]["slow"] == 0 and got[-1]["rounds"]["fast"] == got[-1]["iterations"], got[-1]["rounds"]
    I = np.eye(4, dtype=np.float32)
    off = np.eye(4, dtype=np.float32)
    off[:3, 3] = [0.004, -0.003, 0.02]  # accepts points no sweep accepted before: lazy covariances, deferred chunks
    for j, T in enumerate([off, off, I]):
        _same_sweep(new.debug_correspondences(T, N), old.debug_correspondences(T, N), f"sweep {j}")


def test_gate_change_invalidates_the_lists():
    """A new gate between aligns drops the lists: slow rounds again while they are rebuilt, then fast."""
    scan, cad, _ = _clouds(N, N)
    new, old = _engine(scan, cad), _engine(scan, cad, OLD)
    for _ in range(5):
        a = _align(new)
        _align(old)
    assert a["rounds"]["slow"] == 0 and a["rounds"]["fast"] > 0, a["rounds"]
    for e in (new, old):
        e.setMaxCorrespondenceDistance(0.03)
    got = []
    for k in range(6):
        a, b = _align(new), _align(old)
        _same(a, b, f"align {k + 1} after the gate change")
        got.append(a["rounds"])
    print(got)
    assert got[0]["fast"] == 0 and got[0]["slow"] > 0, got
    assert any(g["pending"] > 0 for g in got[:4]), got
    assert got[-1]["slow"] == 0 and got[-1]["fast"] > 0, got


# ------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("n", [1024, 1025, 1])
def test_chunk_edges(n):
    """One whole chunk, one chunk and a point, a single point (k_correspondences 1: a cloud needs k points)
    against a 5 000-point target: every align and sweep equals the form before r08, whatever it returns."""
    scan, cad, Ttrue = _clouds(N, 5000)
    scan = np.ascontiguousarray(scan[:n])
    prm = {"k": 1} if n == 1 else {}
    new, old = _engine(scan, cad, None, **prm), _engine(scan, cad, OLD, **prm)
    for k in range(6):
        a, b = _align(new), _align(old)
        _same(a, b, f"n {n}, align {k + 1}")
    print(f"n {n}: iterations {a['iterations']}, n_corr {a['n_corr']}, converged {a['converged']}, rounds {a['rounds']}")
    assert a["rounds"]["fast"] > 0 and a["rounds"]["slow"] == 0, a["rounds"]
    Tinv = np.linalg.inv(Ttrue).astype(np.float32)
    for j, T in enumerate([Tinv, Tinv, np.eye(4, dtype=np.float32)]):
        _same_sweep(new.debug_correspondences(T, n), old.debug_correspondences(T, n), f"n {n}, sweep {j}")


def test_rejected_source_leaves_the_context_usable():
    """A source 10 m off the target: no correspondence, the solver's exception (converged false, as PCL
    reports it) in every align, cold and listed; the context then aligns a good source like a fresh one."""
    scan, cad, _ = _clouds(N, N)
    far = np.ascontiguousarray(scan + np.float32([10.0, 0.0, 0.0]))
    new, old = _engine(far, cad), _engine(far, cad, OLD)
    for k in range(5):
        a, b = _align(new), _align(old)
        _same(a, b, f"far source, align {k + 1}")
        assert not a["converged"] and a["n_corr"] < 4, (a["converged"], a["n_corr"])
    print("far source, last align:", a["rounds"])
    for e in (new, old):
        e.set_source_xyz(scan)
    for k in range(5):
        a, b = _align(new), _align(old)
        _same(a, b, f"good source, align {k + 1}")
    assert a["converged"] and a["n_corr"] > N // 2
    assert a["rounds"]["slow"] == 0 and a["rounds"]["fast"] > 0, a["rounds"]
    fresh = _align(_engine(scan, cad))
    np.testing.assert_array_equal(a["T"].view(np.uint32), fresh["T"].view(np.uint32))


def test_profiling_counts_one_correspond_per_sweep():
    """While profiling, kernel_times counts one `correspond` per sweep on both paths, and the aligns are equal."""
    scan, cad, _ = _clouds(N, N)
    new, old = _engine(scan, cad), _engine(scan, cad, OLD)
    for e in (new, old):
        e.set_profiling(True)
    sweeps = 0
    for k in range(5):
        a, b = _align(new), _align(old)
        _same(a, b, f"profiling, align {k + 1}")
        sweeps += a["iterations"]
    assert a["rounds"]["slow"] == 0 and a["rounds"]["fast"] > 0, a["rounds"]
    kn, ko = new.kernel_times(), old.kernel_times()
    assert kn["correspond"]["count"] == ko["correspond"]["count"] == sweeps, (kn, ko, sweeps)
    for e in (new, old):
        e.set_profiling(False)
    _same(_align(new), _align(old), "after profiling")


# ------------------------------------------------------------------------------ the other row paths
def test_ticket_tail_server_equals_launched_passes():
    """"srv_cus" 1 with 163 841 source points: 6 supers on a one-block server of 4 waves, so the server runs
    the ticket tail (more than one super per wave), whose rows the last-arriving waves write; the running total
    waits for them in index order all the same.  Its aligns equal launched passes ("resident" 0)."""
    n = 163841
    scan, cad, _ = _clouds(n, 50000)
    srv, launched = _engine(scan, cad, {"srv_cus": 1}), _engine(scan, cad, {"resident": 0})
    for k in range(3):
        a, b = _align(srv), _align(launched)
        _same(a, b, f"align {k + 1}")
        assert a["passes"]["server_passes"] == a["n_evals"] and a["passes"]["takeovers"] == 0, a["passes"]
        assert b["passes"]["server_launches"] == 0 and b["passes"]["launched_passes"] == b["n_evals"], b["passes"]


def test_takeover_while_the_running_total_waits(monkeypatch):
    """A server whose last block withholds a pass: the host has already added the rows that landed when the
    launched row pass takes over and writes every row again (the same values); the total is the undisturbed
    one.  The rest of the align and the next aligns (which take over again: the knob stalls every server)
    equal those of the form before r08 without the stall."""
    scan, cad, _ = _clouds(N, N)
    ref = _engine(scan, cad, OLD)
    want = [_align(ref) for _ in range(4)]
    ref.close()
    monkeypatch.setenv("MGICP_SRV_STALL_PASS", "1")
    monkeypatch.setenv("MGICP_ROW_DEADLINE_MS", "50")
    e = _engine(scan, cad)
    for k in range(4):
        a = _align(e)
        _same(a, want[k], f"align {k + 1}")
        assert a["passes"]["takeovers"] == 1 and a["passes"]["server_launches"] == 1, a["passes"]
        assert a["passes"]["launched_passes"] == a["n_evals"] - a["passes"]["server_passes"] + 1, a["passes"]
