"""CPU checks of the pass-server parity tests' inputs (tests/pass_server_cases.py): the control-flow
model against hand-worked values, the coverage table (the shape list reaches every named regime of
fdf_server_kernel), and the premises the GPU module builds on, on the oracle alone.  Plus the oracle's
own regression: one RefGICP object given a larger, then a smaller source.
"""
import numpy as np
import pytest

import pass_server_cases as pc


# ------------------------------------------------------------------------------ the model
def test_server_model_hand_worked_values():
    """Three shapes worked by hand from fdf_server_blocks and fdf_server_kernel (nw = 4 blocks; wave w0
    keeps chunk w0 in registers, chunk w0 + nw's first 128 groups in LDS and streams chunks w0 + 2 nw,
    ...; nst = (nch - w1 - 1) / nw; split = (wid nst + 2) / 4; tagged iff nsup <= nw)."""
    # 4609 points on one block: 5 chunks, the fifth (513 points = 129 groups of 4) is wave 0's LDS chunk:
    # 128 groups from LDS, one streamed
    m = pc.server_model(4609, 1)
    assert (m.nch, m.blocks, m.nw, m.nsup, m.servable, m.tagged) == (5, 1, 4, 1, True, True)
    assert (m.reg_chunks, m.lds_chunks, m.streamed_chunks) == ([0, 1, 2, 3], [4], [])
    assert m.fill == [1024, 1024, 1024, 1024, 513] and m.groups[4] == 129
    assert (m.lds_groups, m.lds_rest_groups) == ([129], [1])
    assert [w.nmine for w in m.waves] == [2, 1, 1, 1] and m.idle_waves == 0 and m.last_nin == 5
    assert m.nst == [0] and m.split == [0]
    # 21504 points on one block: 21 full chunks; wave 0 streams 8, 12, 16, 20 (nst 4, split 0), wave 1
    # 9, 13, 17 (nst 3, split (3 + 2) / 4 = 1), wave 2 10, 14, 18 (split (6 + 2) / 4 = 2), wave 3 11, 15, 19
    # (split (9 + 2) / 4 = 2)
    m = pc.server_model(21504, 1)
    assert (m.nch, m.nw, m.nsup, m.tagged, m.last_nin) == (21, 4, 1, True, 21)
    assert m.lds_chunks == [4, 5, 6, 7] and m.streamed_chunks == list(range(8, 21))
    assert [w.streamed for w in m.waves] == [[8, 12, 16, 20], [9, 13, 17], [10, 14, 18], [11, 15, 19]]
    assert [(w.nst, w.split, w.nmine) for w in m.waves] == [(4, 0, 6), (3, 1, 5), (3, 2, 5), (3, 2, 5)]
    # 393217 points on three blocks: 385 chunks (the last holds one point) on 12 waves, 13 supers > 12
    # waves: untagged; wave 0 holds chunks 0, 12, ..., 384 (33: 31 streamed), wave 1 1, 13, ..., 373 (32)
    m = pc.server_model(393217, 3)
    assert (m.nch, m.blocks, m.nw, m.nsup) == (385, 3, 12, 13)
    assert (m.servable, m.tagged, m.untagged, m.last_nin, m.fill[-1]) == (True, False, True, 1, 1)
    assert m.waves[0].streamed == list(range(24, 385, 12)) and (m.waves[0].nst, m.waves[0].nmine) == (31, 33)
    assert (m.waves[1].nst, m.waves[1].nmine, m.waves[1].streamed[-1]) == (30, 32, 373)
    assert m.waves[5].wid == 1 and m.waves[5].split == (1 * 30 + 2) // 4 and m.max_nmine == 33
    # and the limit: 257 chunks are one too many for 4 waves of 64 tickets, 256 are not
    assert not pc.server_model(262145, 1).servable and pc.server_model(262144, 1).servable
    assert pc.server_model(262145, 1).blocks == 1 and pc.server_model(262145, 2).servable
    # fewer chunks than waves: a block per 4 chunks, not per CU
    assert pc.server_model(4097, 3).blocks == 2 and pc.server_model(1, 3).blocks == 1


def test_model_fill_changes_groups_only():
    m = pc.server_model(5 * 1024, 1, fill=[0, 1, 4, 5, 1024])
    assert m.groups == [0, 1, 1, 2, 256] and m.reg_groups == [0, 1, 1, 2] and m.lds_groups == [256]
    assert (m.nch, m.nw, m.nsup) == (5, 4, 1)


def test_shape_list_reaches_every_named_regime():
    """the coverage table: every shape is in each regime it is listed for, and every regime of the
    server's control flow is reached by at least one shape"""
    reached = set()
    for (ns, cus), regimes in pc.SHAPES.items():
        m = pc.server_model(ns, cus)
        for r in regimes:
            assert pc.REGIMES[r](m), (ns, cus, r)
        reached |= {r for r, pred in pc.REGIMES.items() if pred(m)}
    claimed = {r for regimes in pc.SHAPES.values() for r in regimes}
    assert claimed == set(pc.REGIMES), sorted(set(pc.REGIMES) - claimed)
    assert reached == set(pc.REGIMES)
    # the shapes of the narrower test families are shapes of the list
    for fam in (pc.RUN_SHAPES, pc.FORM_SHAPES, pc.ALIGN_SHAPES, pc.TAKEOVER_SHAPES):
        assert set(fam) <= set(pc.SHAPES)
    # take-overs: one untagged shape, one tagged shape that streams
    m_u, m_t = (pc.server_model(*s) for s in pc.TAKEOVER_SHAPES)
    assert m_u.untagged and m_t.tagged and m_t.streamed_chunks
    # the live-server runs: tagged with one and two supers, untagged at its first and its last shape
    assert [pc.server_model(*s).tagged for s in pc.RUN_SHAPES] == [True, True, False, False]
    # forms: device-total tickets (host_rows 0) over an LDS remainder, streamed chunks and several supers
    assert [pc.server_model(*s).nsup for s in pc.FORM_SHAPES] == [1, 1, 5]
    # both slabs: 21 chunks on one block -- 4 register, 4 LDS and 13 streamed chunks
    m = pc.server_model(pc.SLAB_NS, 1)
    assert (m.nch, len(m.reg_chunks), len(m.lds_chunks), len(m.streamed_chunks)) == (21, 4, 4, 13)
    assert 0 < m.fill[-1] < pc.CHUNK_PTS
    # row stamps of consecutive passes alternate: six passes use both parity buffers three times
    assert len(pc.RUN_STATES) == 6 and pc.RUN_STATES[0] == pc.RUN_STATES[3] == pc.RUN_STATES[4]


# ------------------------------------------------------------------------------ the premises
@pytest.mark.parametrize("ns", [1, 4353, 262145])
def test_full_pair_accepts_every_source_point(ns):
    o, m, tj = pc.oracle("full", ns)
    assert m == ns and (tj >= 0).all()
    assert pc.chunk_fill(tj, np.arange(ns)) == pc.server_model(ns, 1).fill


@pytest.mark.parametrize("which", pc.SLABS)
def test_slab_is_exactly_what_the_gate_rejects(which):
    src, tgt, Ttrue, gate, moved = pc.slab_pair(which)
    assert len(src) == pc.SLAB_NS and moved.sum() == pc.SLAB_PTS >= 8 * pc.CHUNK_PTS
    assert gate == pc.SLAB_GATE
    # the slab is a run of the index (= z) order, clear of the rest by half a metre: no grid layer holds both
    assert (np.diff(src[:, 2]) >= 0).all()
    run = np.flatnonzero(moved)
    assert run[-1] - run[0] + 1 == pc.SLAB_PTS
    if which == "high":
        assert run[-1] == len(src) - 1 and src[run[0], 2] - src[run[0] - 1, 2] >= 0.4999
    else:
        assert run[0] == 0 and src[run[-1] + 1, 2] - src[run[-1], 2] >= 0.4999
    o, m, tj = pc.oracle(which)
    np.testing.assert_array_equal(tj < 0, moved)  # exactly the slab
    assert m == pc.SLAB_NS - pc.SLAB_PTS
    prof = pc.chunk_fill(tj, np.arange(len(src)))  # accepted per 1024 of the index order
    zeros = "".join("0" if c == 0 else "x" for c in prof)
    assert "0" * 8 in zeros, prof
    assert any(0 < c < pc.CHUNK_PTS for c in prof[:-1]), prof  # the mixed seam (not just the short last chunk)
    assert (prof[0] == 0) == (which == "low") and (prof[-1] == 0) == (which == "high")


# ------------------------------------------------------------------------------ the oracle itself
def test_oracle_object_reused_across_source_sizes():
    """ref_correspondences kept the sweep's buffers of the FIRST source it saw: a larger source on the
    same object overflowed them (heap overflow, a segmentation fault at 4353 -> 262145 points).
    ref_set_source now drops them.  One object, a growing and then a shrinking source: the sweep and
    the tree sums equal a fresh object's."""
    from oracle import ref

    x = np.array(pc.X_SMALL)

    def sweep(o, ns):
        src, tgt, Ttrue, gate = pc.full_pair(ns)
        assert o.set_source(src) == 0
        m, tj, d2, M = o.correspondences(pc.sweep_transform(Ttrue))
        o.set_sum_order(1, np.arange(ns, dtype=np.uint32))
        return m, tj, d2, M, o.fdf_mode_sums(x), o.fdf(x)

    def new():
        o = ref.RefGICP(max_corr_dist=pc.FULL_GATE)
        o.set_target(pc.full_pair(1)[1])
        o.set_mahalanobis_upper(True)
        return o

    reused = new()
    for ns in (4353, 262145, 4097):
        a, b = sweep(reused, ns), sweep(new(), ns)
        assert a[0] == b[0] == ns
        for u, v in zip(a[1:5], b[1:5]):
            np.testing.assert_array_equal(u, v)
        assert a[5][0] == b[5][0]
        np.testing.assert_array_equal(a[5][1], b[5][1])
    # a sweep is needed again after a new source: the old one's correspondences are gone with it
    src, tgt, Ttrue, gate = pc.full_pair(1000)
    reused.set_source(src)
    assert reused.lib.ref_fdf_mode_sums(reused.h, ref._dp(x), ref._dp(np.zeros(14))) != 0
