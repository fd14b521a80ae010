"""The resident pass server (fdf_server_kernel) against the CPU oracle's restatement of the engine's fixed
reduction tree, BIT FOR BIT, at every regime of its control flow.

The server's control flow depends on the ratio of chunks to server waves (nw = 4 x blocks): which chunk a
wave keeps in registers, which in LDS, how many it streams and in what order, whether wave s reduces
super s from stamped chunk partials ("tagged", nsup <= nw) or the waves draw chunk tickets counted modulo
the supers' sizes ("untagged"), and whether the shard is servable at all (nch <= 64 nw).  On a 256-CU
device nw is 1024, so every test below a million points keeps every chunk in registers and the untagged
path needs 33.5M source points.  Debug option "srv_cus" caps the server's blocks: with 1 to 3 blocks
every regime is reached between 1 and 393 217 points (tests/pass_server_cases.py: the shape list, the
clouds, and the model that certifies which shape reaches which branch; tests/test_pass_server_inputs.py
checks those on the CPU).

Every comparison is exact (array_equal): the oracle runs the engine's tree (ref_set_sum_order 1) over the
engine's own stream order with the engine's 6-entry Mahalanobis storage (DESIGN.md "Numerics").
"""
import time

import numpy as np
import pytest

import pass_server_cases as pc

pytestmark = pytest.mark.gpu

CASES = [("full", ns, cus) for (ns, cus) in pc.SHAPES] + [(w, pc.SLAB_NS, 1) for w in pc.SLABS]


def _id(case):
    return f"{case[0]}-{case[1]}-{case[2]}"


_OF_THE_TEST = []  # engines a test built: closed when it ends, passed or not (see _close_the_tests_engines)


def _engine(name, ns, cus, **opts):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    src, tgt, Ttrue, gate = pc.pair(name, ns)
    e = GICPEngine(max_corr_dist=gate, k=pc.knn_k(len(src)),
                   options={"target_cache": 0, "srv_cus": cus, **opts})
    _OF_THE_TEST.append(e)
    e.set_source_xyz(src)
    e.set_target_xyz(tgt)
    return e


class _Setup:
    """engine and oracle of one case after the same sweep at inv(Ttrue), the oracle on the engine's tree"""

    def __init__(self, name, ns, cus, **opts):
        self.case = (name, ns, cus)
        src, tgt, Ttrue, gate = pc.pair(name, ns)
        self.n = len(src)
        self.T = pc.sweep_transform(Ttrue)
        self.e = _engine(name, ns, cus, **opts)
        self.order = self.e.debug_source_order(self.n)
        assert len(self.order) == self.n and np.array_equal(np.sort(self.order), np.arange(self.n))
        self.o, self.m, self.tj = pc.oracle(name, ns)
        self.o.set_sum_order(1, self.order)
        m_e, tj_e, _ = self.e.debug_correspondences(self.T, self.n)
        assert m_e == self.m, (m_e, self.m)
        np.testing.assert_array_equal(tj_e, self.tj)  # the same matches: the passes sum the same terms
        self.fill = pc.chunk_fill(self.tj, self.order)
        self.model = pc.server_model(self.n, cus, self.fill)

    def close(self):
        self.e.close()


@pytest.fixture(autouse=True)
def _close_the_tests_engines():
    """a context that ran a server holds the device's one server slot until it is drained or destroyed: an
    engine left open by a failed assertion must not turn the next test's server into launched passes"""
    yield
    while _OF_THE_TEST:
        _OF_THE_TEST.pop().close()


@pytest.fixture(scope="module", params=CASES, ids=_id)
def case_setup(request):
    s = _Setup(*request.param)
    _OF_THE_TEST.remove(s.e)  # lives as long as the case
    yield s
    s.close()


@pytest.fixture
def ctx(case_setup):
    """the case's engine and oracle, shared by the tests of the case; after each test the engine's stream
    is drained, which gives the device's one server slot back (a context keeps it until then) to the
    engines the other tests build"""
    yield case_setup
    case_setup.e.debug_option("srv_cus", case_setup.case[2])


def _delta(e, before):
    after = e.pass_stats()
    assert after["server_denied"] == 0, after  # no other context of the process holds the device's server slot
    return {k: after[k] - before[k] for k in ("server_launches", "server_passes", "launched_passes", "takeovers")}


def SERVED(n):  # n hooks that each launched a server for their one pass
    return {"server_launches": n, "server_passes": n, "launched_passes": 0, "takeovers": 0}


def LAUNCHED(n):
    return {"server_launches": 0, "server_passes": 0, "launched_passes": n, "takeovers": 0}


# ------------------------------------------------------------------------------ premise
def test_shape_is_in_the_regime_the_table_claims(ctx):
    """The accepted correspondences per chunk, from the oracle's matches in the ENGINE's stream order,
    put the shape where the table says (the model with the real fill, not the nominal one)."""
    name, ns, cus = ctx.case
    m = ctx.model
    print(f"{_id(ctx.case)}: nch {m.nch} nw {m.nw} nsup {m.nsup} tagged {m.tagged} servable {m.servable} "
          f"nst {m.nst} split {m.split} nmine {m.max_nmine} last nin {m.last_nin} idle {m.idle_waves} fill {m.fill[:24]}")
    if name == "full":
        assert ctx.m == ns and m.fill == pc.server_model(ns, cus).fill
        for r in pc.SHAPES[(ns, cus)]:
            assert pc.REGIMES[r](m), r
        return
    reg = [m.fill[j] for j in m.reg_chunks]
    lds = [m.fill[j] for j in m.lds_chunks]
    stream = [m.fill[j] for j in m.streamed_chunks]
    assert m.tagged and ctx.m == pc.SLAB_NS - pc.SLAB_PTS
    assert sum(c == 0 for c in m.fill) >= 8 and any(0 < c < pc.CHUNK_PTS for c in m.fill[:-1]), m.fill
    if name == "low":  # the slab sorts first: wholly rejected register, LDS and streamed chunks
        assert 0 in reg and 0 in lds and 0 in stream, m.fill
        assert m.fill[:8] == [0] * 8
    else:              # the slab sorts last: the wholly rejected chunks are streamed ones
        assert 0 not in reg and 0 not in lds and stream.count(0) >= 8, m.fill
        assert m.fill[-8:] == [0] * 8


# ------------------------------------------------------------------------------ single passes
def test_single_passes_equal_the_oracle_tree(ctx):
    """mgicp_debug_fdf_sums / mgicp_debug_fdf (one server launch per pass) at a zero state, the suite's
    small state and a 0.5 rad rotation; the counters prove which path ran."""
    e, o, served = ctx.e, ctx.o, ctx.model.servable
    for x in pc.STATES:
        x = np.array(x)
        before = e.pass_stats()
        s = e.debug_fdf_sums(x)
        assert _delta(e, before) == (SERVED(1) if served else LAUNCHED(1)), (x, _delta(e, before))
        np.testing.assert_array_equal(s[:14], o.fdf_mode_sums(x), err_msg=f"{_id(ctx.case)} x = {x}")
        assert s[13] == ctx.m
        before = e.pass_stats()
        f_e, g_e = e.debug_fdf(x)
        assert _delta(e, before) == (SERVED(1) if served else LAUNCHED(1))
        f_o, g_o = o.fdf(x)
        assert f_e == f_o, (f_e, f_o)
        np.testing.assert_array_equal(g_e, g_o)
    if not served:
        assert e.pass_stats()["server_launches"] == 0


def test_launched_passes_equal_the_oracle_tree(ctx):
    """the control: a "resident" 0 engine (fdf_soa_kernel) at both sweep directions"""
    name, ns, cus = ctx.case
    f = _engine(name, ns, cus, resident=0)
    f.debug_correspondences(ctx.T, ctx.n)
    for x in pc.STATES:
        x = np.array(x)
        want = ctx.o.fdf_mode_sums(x)
        before = f.pass_stats()
        a, b = f.debug_fdf_sums(x), f.debug_fdf_sums(x)  # consecutive passes: opposite directions
        assert _delta(f, before) == LAUNCHED(2)
        np.testing.assert_array_equal(a[:14], want)
        np.testing.assert_array_equal(b[:14], want)


def test_timing_form_equals_the_oracle_tree(ctx):
    """mgicp_debug_pass_bench: five passes of one server launch chained on the device (mode 0) and five
    launched passes (mode 1)"""
    from leica_point_cloud_processing_amd import _lib

    x = np.array(pc.X_SMALL)
    want = ctx.o.fdf_mode_sums(x)
    ms1, s1 = ctx.e.debug_pass_bench(x, 5, 1)
    np.testing.assert_array_equal(s1[:14], want)
    if not ctx.model.servable:
        with pytest.raises(_lib.MgicpError):
            ctx.e.debug_pass_bench(x, 5, 0)
        return
    ms0, s0 = ctx.e.debug_pass_bench(x, 5, 0)
    print(f"{_id(ctx.case)}: server {1e3 * ms0:.1f} us / pass on {ctx.model.blocks} block(s), launched {1e3 * ms1:.1f} us")
    np.testing.assert_array_equal(s0[:14], want)
    np.testing.assert_array_equal(ctx.e.debug_fdf_sums(x)[:14], want)  # and the command path after it
    assert ctx.e.pass_stats()["takeovers"] == 0


# ------------------------------------------------------------------------------ one live server
RUN_CASES = [("full", ns, cus) for (ns, cus) in pc.RUN_SHAPES] + [(w, pc.SLAB_NS, 1) for w in pc.SLABS]


@pytest.mark.parametrize("case", RUN_CASES, ids=_id)
def test_six_passes_on_one_live_server(case):
    """mgicp_debug_fdf_sums_run: ONE server launch serves six passes (the other hooks tear the server down
    after each) -- resident chunks reused at new states, a repeated state, both parities of the row
    buffers, and in the untagged path tickets that keep counting modulo the supers' sizes."""
    s = _Setup(*case)
    xs = np.array(pc.RUN_STATES)
    before = s.e.pass_stats()
    t0 = time.perf_counter()
    got = s.e.debug_fdf_sums_run(xs)
    dt = time.perf_counter() - t0
    d = _delta(s.e, before)
    print(f"{_id(case)}: six passes on one server in {1e3 * dt:.1f} ms, {d}")
    assert d == {"server_launches": 1, "server_passes": 6, "launched_passes": 0, "takeovers": 0}, d
    for k, x in enumerate(xs):
        np.testing.assert_array_equal(got[k, :14], s.o.fdf_mode_sums(x), err_msg=f"{_id(case)} pass {k}")
    np.testing.assert_array_equal(got[0], got[3])
    np.testing.assert_array_equal(got[3], got[4])
    # and once more on the same context: a second server behind the first one's cancel
    np.testing.assert_array_equal(s.e.debug_fdf_sums_run(xs), got)
    assert _delta(s.e, before)["server_launches"] == 2


# ------------------------------------------------------------------------------ server forms
@pytest.mark.parametrize("bar,rows", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", pc.FORM_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_server_forms_give_identical_sums(shape, bar, rows):
    """commands through the BAR or the pinned copy x super partials as host rows or the device total
    ("host_rows" 0: wave_tickets' device-total path, re-armed tickets, at 4 waves)"""
    s = _Setup("full", shape[0], shape[1], bar_cmd=bar, host_rows=rows)
    xs = np.array(pc.RUN_STATES)
    before = s.e.pass_stats()
    got = s.e.debug_fdf_sums_run(xs)
    one = s.e.debug_fdf_sums(xs[2])
    d = _delta(s.e, before)
    st = s.e.pass_stats()
    assert d == {"server_launches": 2, "server_passes": 7, "launched_passes": 0, "takeovers": 0}, d
    assert st["row_allocs"] == rows and st["bar_commands"] == bar, st
    for k, x in enumerate(xs):
        np.testing.assert_array_equal(got[k, :14], s.o.fdf_mode_sums(x), err_msg=f"pass {k}")
    np.testing.assert_array_equal(one, got[2])


# ------------------------------------------------------------------------------ aligns
ALIGN_CASES = [("full", ns, cus) for (ns, cus) in pc.ALIGN_SHAPES] + [("low", pc.SLAB_NS, 1)]


def _align(e):
    T = e.align()
    r = e.last_result
    return T, r["iterations"], r["n_evals"], r["n_corr"], [np.asarray(t, np.float32) for t in e.debug_trace(200)]


def _same_align(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    assert a[1:4] == b[1:4], (what, a[1:4], b[1:4])
    assert len(a[4]) == len(b[4]), what
    for u, v in zip(a[4], b[4]):
        np.testing.assert_array_equal(u, v, err_msg=what)


@pytest.mark.parametrize("case", ALIGN_CASES, ids=_id)
def test_aligns_equal_the_oracle_and_launched_passes(case):
    """whole aligns through a small server: T, iterations, device passes and every per-iteration transform
    equal a "resident" 0 engine's, and T, iterations, the last sweep's count and every per-iteration
    transform the oracle's align on the engine's tree, bit for bit; one server per outer iteration; a second
    align on the context repeats the first.  The oracle's n_evals counts every call of PCL's functor (f, df
    and fdf are separate calls: 111 / 191 / 153 / 254 at these four cases), the engine's the device passes
    left after its memo of the last state (64 / 118 / 90 / 160): the two are different quantities, so the
    evaluation count is compared with the launched engine only."""
    name, ns, cus = case
    e = _engine(name, ns, cus)
    order = e.debug_source_order(len(pc.pair(name, ns)[0]))
    first = _align(e)
    st = e.pass_stats()
    assert st["server_launches"] == first[1] and st["server_passes"] == first[2], (st, first[1:4])
    assert st["launched_passes"] == 0 and st["takeovers"] == 0, st
    second = _align(e)
    _same_align(second, first, "second align on the context")
    assert e.pass_stats()["server_launches"] == 2 * first[1]
    e.close()
    f = _engine(name, ns, cus, resident=0)
    launched = _align(f)
    assert f.pass_stats()["server_launches"] == 0
    f.close()
    _same_align(launched, first, "launched passes")
    o, _, _ = pc.oracle(name, ns)
    o.set_sum_order(1, order)
    T_o, info = o.align(want_trace=True)
    pc.oracle_stale(name, ns)
    print(f"{_id(case)}: iterations {first[1]} (oracle {info['iterations']}), evaluations {first[2]} "
          f"(oracle {info['n_evals']}), n_corr {first[3]} (oracle {info['n_corr_last']})")
    assert info["converged"] == 1
    np.testing.assert_array_equal(T_o, first[0])
    assert (info["iterations"], info["n_corr_last"]) == (first[1], first[3])
    assert info["n_evals"] >= first[2]
    assert len(info["trace"]) == len(first[4])
    for u, v in zip(info["trace"], first[4]):
        np.testing.assert_array_equal(np.asarray(u, np.float32), v)


# ------------------------------------------------------------------------------ take-over
# an untagged and a streamed tagged shape on one block (its only block is the last one: the stalled pass is
# withheld whole), and the untagged shape on two blocks, where block 0 has drawn its tickets of the stalled
# pass and block 1 has not: the take-over finds every super's ticket half counted
TAKEOVER_CASES = list(pc.TAKEOVER_SHAPES) + [(262145, 2)]


@pytest.mark.parametrize("shape", TAKEOVER_CASES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_takeover_of_a_small_server(monkeypatch, shape):
    """MGICP_SRV_STALL_PASS 1: the last block withholds the second pass of every server, the host takes the
    pass over after the (shortened) row deadline and the rest of the align runs launched passes:
    T, iterations and evaluations are the undisturbed align's, one take-over per align.  The second pass
    of a BFGS run is a line-search trial: an align can come out the same although that one pass summed the
    wrong chunks (seen with a scratch build whose host-row super sum dropped a chunk, at 13312 points),
    so the taken-over pass's own sums are compared with the oracle first."""
    ns, cus = shape
    ref = _engine("full", ns, cus)
    want = _align(ref)
    assert ref.pass_stats()["takeovers"] == 0
    ref.close()
    monkeypatch.setenv("MGICP_SRV_STALL_PASS", "1")
    monkeypatch.setenv("MGICP_ROW_DEADLINE_MS", "50")
    # the withheld pass itself: pass 1 of six on one server is the launched take-over pass, writing the
    # server's rows with the server's stamp -- its sums, like every other pass's, are the oracle's
    s = _Setup("full", ns, cus)
    xs = np.array(pc.RUN_STATES)
    got = s.e.debug_fdf_sums_run(xs)
    st = s.e.pass_stats()
    assert (st["takeovers"], st["server_launches"], st["server_passes"], st["launched_passes"]) == (1, 1, 2, 5), st
    for k, x in enumerate(xs):
        np.testing.assert_array_equal(got[k, :14], s.o.fdf_mode_sums(x), err_msg=f"pass {k}")
    s.close()
    e = _engine("full", ns, cus)
    for k in range(2):
        got = _align(e)
        _same_align(got, want, f"align {k} with a withheld pass")
        st = e.pass_stats()
        assert st["takeovers"] == k + 1, st
        assert st["server_launches"] == k + 1, st  # degraded after the take-over: no more servers
        assert st["launched_passes"] == (k + 1) * want[2] - st["server_passes"] + st["takeovers"], st
    e.close()
