"""Shapes, clouds and the control-flow model of the resident pass server's parity tests.

Shared by tests/test_pass_server_inputs.py (CPU: the model against hand-worked values, the coverage
table, the oracle's premises) and tests/test_pass_server_gpu.py (engine vs oracle, bit for bit).
Nothing here touches the engine.  Every builder is cached: a cloud is made once per process and must
not be modified.

server_model restates, from the formulas of fdf_server_blocks and fdf_server_kernel
(csrc/mgicp_kernels.hip), which chunk of a shard a server wave keeps in registers, which in LDS, which
it streams and in what order, and how the supers are reduced.  It SELECTS and CERTIFIES inputs -- "this
shape reaches that branch" -- and is never a reference for a sum: every sum is compared with the CPU
oracle's restatement of the fixed reduction tree (oracle/gicp_ref.c fdf_tree).
"""
import functools
from types import SimpleNamespace

import numpy as np

CHUNK_PTS = 1024     # kChunkPts: one wave sums one chunk of the grid-sorted source
SUPER_CHUNKS = 32    # kSuperChunks
SRV_WAVES = 4        # kSrvWaves: the server's block, one wave per SIMD
REG_GROUPS = 4       # kR: groups of 4 correspondences per lane kept in registers (a whole chunk)
LDS_GROUPS = 2       # kL: groups per lane of the wave's second chunk kept in LDS
MAX_TICKETS = 64     # a wave's lanes draw the tickets of all its chunks at once


def server_model(ns: int, srv_cus: int, fill=None) -> SimpleNamespace:
    """The server's control flow for a shard of `ns` source points on at most `srv_cus` blocks.
    `fill`: accepted correspondences per chunk of the stream order (default: every point accepted,
    chunk j holds min(1024, ns - 1024 j))."""
    nch = -(-ns // CHUNK_PTS)
    nb = min(srv_cus, -(-nch // SRV_WAVES)) if nch and srv_cus > 0 else 0  # fdf_server_blocks
    nw = SRV_WAVES * nb
    servable = nb > 0 and nch <= MAX_TICKETS * nw
    nsup = -(-nch // SUPER_CHUNKS)
    if fill is None:
        fill = [min(CHUNK_PTS, ns - CHUNK_PTS * j) for j in range(nch)]
    fill = [int(c) for c in fill]
    assert len(fill) == nch and all(0 <= c <= CHUNK_PTS for c in fill)
    groups = [(c + 3) // 4 for c in fill]  # chunk_g1 - chunk_g0
    waves = []
    for w0 in range(nw):
        wid, w1 = w0 % SRV_WAVES, w0 + nw
        nst = (nch - w1 - 1) // nw if w1 + nw < nch else 0
        waves.append(SimpleNamespace(
            w0=w0, wid=wid, reg=w0 if w0 < nch else None, lds=w1 if w1 < nch else None,
            streamed=list(range(w1 + nw, nch, nw)), nst=nst, split=(wid * nst + SRV_WAVES // 2) // SRV_WAVES,
            nmine=-(-(nch - w0) // nw) if w0 < nch else 0))
        assert len(waves[-1].streamed) == nst
    reg = [w.reg for w in waves if w.reg is not None]
    lds = [w.lds for w in waves if w.lds is not None]
    streamed = sorted(j for w in waves for j in w.streamed)
    assert not nw or sorted(reg + lds + streamed) == list(range(nch))
    return SimpleNamespace(
        ns=ns, srv_cus=srv_cus, nch=nch, blocks=nb, nw=nw, nsup=nsup, servable=servable,
        tagged=servable and nsup <= nw, untagged=servable and nsup > nw,
        reg_chunks=reg, lds_chunks=lds, streamed_chunks=streamed, waves=waves,
        nst=sorted({w.nst for w in waves if w.reg is not None}),
        split=sorted({w.split for w in waves if w.reg is not None}),
        max_nmine=max((w.nmine for w in waves), default=0),
        last_nin=nch - SUPER_CHUNKS * (nsup - 1) if nch else 0,
        idle_waves=sum(w.reg is None for w in waves),
        fill=fill, groups=groups,
        reg_groups=[groups[j] for j in reg],
        # an LDS chunk's groups: the first 2 per lane (128) come from LDS, the rest are streamed
        lds_groups=[groups[j] for j in lds],
        lds_rest_groups=[max(0, groups[j] - LDS_GROUPS * 64) for j in lds],
        streamed_groups=[groups[j] for j in streamed])


# ---------------------------------------------------------------------------------- regimes
# name -> predicate on the model; the CPU module asserts every claim of SHAPES and that every regime
# below is claimed by at least one shape
REGIMES = {
    "one_chunk": lambda m: m.nch == 1,
    "idle_3": lambda m: m.servable and m.idle_waves == 3,
    "idle_beside_working": lambda m: m.servable and m.blocks > 1 and 0 < m.idle_waves < m.nw,
    "reg_partial": lambda m: m.servable and any(0 < c < CHUNK_PTS for c in (m.fill[j] for j in m.reg_chunks)),
    "reg_only": lambda m: m.servable and not m.lds_chunks and m.idle_waves == 0,
    "lds_1_group": lambda m: m.servable and 1 in m.lds_groups,
    "lds_64_groups": lambda m: m.servable and 64 in m.lds_groups,      # the first LDS slot exactly full
    "lds_65_groups": lambda m: m.servable and 65 in m.lds_groups,      # the second LDS slot is used
    "lds_128_groups": lambda m: m.servable and 128 in m.lds_groups,    # both slots full, nothing streamed
    "lds_129_groups": lambda m: m.servable and 129 in m.lds_groups,    # the first streamed remainder
    "lds_full": lambda m: m.servable and 256 in m.lds_groups,          # a full LDS chunk
    "all_waves_lds": lambda m: m.servable and len(m.lds_chunks) == m.nw,
    "no_stream": lambda m: m.servable and len(m.lds_chunks) == m.nw and not m.streamed_chunks,
    "stream_1_point": lambda m: m.servable and any(m.fill[j] == 1 for j in m.streamed_chunks),
    "stream_partial": lambda m: m.servable and any(1 < m.fill[j] < CHUNK_PTS for j in m.streamed_chunks),
    "nst_1_2": lambda m: m.servable and {1, 2} <= set(m.nst),
    "nst_3_4": lambda m: m.servable and {3, 4} <= set(m.nst),
    "split_0_1": lambda m: m.servable and {0, 1} <= set(m.split),
    "split_0_1_2": lambda m: m.servable and {0, 1, 2} <= set(m.split),
    "one_full_super": lambda m: m.servable and m.nsup == 1 and m.last_nin == SUPER_CHUNKS,
    "second_super_1_chunk": lambda m: m.tagged and m.nsup == 2 and m.last_nin == 1 and m.fill[-1] == 1,
    "two_supers_tagged": lambda m: m.tagged and m.nsup == 2,
    "last_tagged": lambda m: m.tagged and m.nsup == m.nw,
    "first_untagged": lambda m: m.untagged and m.nsup == m.nw + 1,
    "untagged": lambda m: m.untagged,
    "untagged_last_nin_1": lambda m: m.untagged and m.last_nin == 1,
    "nmine_33": lambda m: m.untagged and m.max_nmine == 33,
    "untagged_partial_last": lambda m: m.untagged and 0 < m.fill[-1] < CHUNK_PTS,
    "nmine_64": lambda m: m.untagged and m.max_nmine == MAX_TICKETS and m.nch == MAX_TICKETS * m.nw,
    "unservable": lambda m: m.nch > 0 and m.blocks > 0 and not m.servable,
    "odd_blocks": lambda m: m.servable and m.blocks == 3,
    "one_lds_chunk": lambda m: m.servable and len(m.lds_chunks) == 1,
    "two_blocks": lambda m: m.servable and m.blocks == 2,
    "three_blocks": lambda m: m.servable and m.blocks == 3,
}

# (ns, srv_cus) -> the regimes the shape is in the list for
SHAPES = {
    (1, 1): ("one_chunk", "idle_3", "reg_partial"),
    (1000, 1): ("one_chunk", "reg_partial"),
    (4096, 1): ("reg_only",),
    (4097, 1): ("lds_1_group", "one_lds_chunk"),
    (4352, 1): ("lds_64_groups",),
    (4353, 1): ("lds_65_groups",),
    (4608, 1): ("lds_128_groups",),
    (4609, 1): ("lds_129_groups",),
    (5120, 1): ("lds_full",),
    (8192, 1): ("all_waves_lds", "no_stream"),
    (8193, 1): ("stream_1_point",),
    (13312, 1): ("nst_1_2", "split_0_1"),
    (21504, 1): ("nst_3_4", "split_0_1_2"),
    (32768, 1): ("one_full_super",),
    (32769, 1): ("second_super_1_chunk",),
    (131072, 1): ("last_tagged",),
    (131073, 1): ("first_untagged", "untagged_last_nin_1", "nmine_33"),
    (163340, 1): ("untagged", "untagged_partial_last"),
    (262144, 1): ("untagged", "nmine_64"),
    (262145, 1): ("unservable",),
    (4097, 2): ("idle_beside_working", "two_blocks"),
    (262145, 2): ("untagged", "two_blocks"),
    (13312, 3): ("odd_blocks", "one_lds_chunk"),
    (25605, 3): ("three_blocks", "all_waves_lds", "stream_partial"),
    (36941, 3): ("three_blocks", "two_supers_tagged"),
    (393217, 3): ("three_blocks", "untagged"),
}

RUN_SHAPES = ((13312, 1), (36941, 3), (131073, 1), (262144, 1))   # several passes on one live server
FORM_SHAPES = ((4609, 1), (13312, 1), (163340, 1))                 # bar_cmd x host_rows
ALIGN_SHAPES = ((13312, 1), (163340, 1), (36941, 3))               # + the "low" slab
TAKEOVER_SHAPES = ((163340, 1), (13312, 1))                        # untagged, streamed tagged

# ---------------------------------------------------------------------------------- states
X_ZERO = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
X_SMALL = (0.001, -0.002, 0.0005, 0.0003, -0.0002, 0.0004)  # the suite's usual small state
X_ROT = (0.003, 0.001, -0.002, 0.5, -0.1, 0.2)              # a 0.5 rad rotation
STATES = (X_ZERO, X_SMALL, X_ROT)
# six passes of one live server: a repeated state, both parities of the row stamp at every state kind
RUN_STATES = (X_SMALL, X_ZERO, X_ROT, X_SMALL, X_SMALL, (-0.002, 0.0015, 0.001, -0.0004, 0.0006, -0.0003))

# ---------------------------------------------------------------------------------- clouds
FULL_NS_MAX = 393217
FULL_NT = 20000
FULL_GATE = 5.0   # metres: wider than the part, so every source point has a partner
SLAB_GATE = 0.04  # the engine's and PCL's default
SLAB_NT = 100000  # dense enough that the gate accepts every scan point left in place (see slab_pair)
SLAB_CHUNKS = 21
SLAB_NS = SLAB_CHUNKS * CHUNK_PTS - 500   # the last chunk partly filled
SLAB_PTS = 9 * CHUNK_PTS + 300            # >= 8 chunks wholly rejected wherever the slab sorts, a mixed one at its seam
SLAB_SHIFT = 0.5                          # metres between the slab and the rest of the scan, along z


@functools.lru_cache(maxsize=None)
def _full_clouds():
    from leica_point_cloud_processing_amd import synth

    return synth.scan_vs_cad(FULL_NS_MAX, FULL_NT)


def full_pair(ns: int):
    """(source, target, Ttrue, gate): the first `ns` points of one 393 217-point scan against 20 000 CAD
    points at a 5 m gate -- the oracle accepts every source point (tests/test_pass_server_inputs.py), so
    chunk j of the stream order holds exactly min(1024, ns - 1024 j) correspondences"""
    scan, cad, Ttrue = _full_clouds()
    assert 1 <= ns <= len(scan)
    return np.ascontiguousarray(scan[:ns]), cad, Ttrue, FULL_GATE


@functools.lru_cache(maxsize=None)
def _slab_clouds():
    from leica_point_cloud_processing_amd import synth

    return synth.scan_vs_cad(SLAB_NS, SLAB_NT)


@functools.lru_cache(maxsize=None)
def slab_pair(which: str):
    """(source, target, Ttrue, gate, moved mask): tests/geometry_edges_cases.py split_source at 21 chunks.
    The scan with a slab of SLAB_PTS of its points displaced along z until the slab clears the whole scan
    by 0.5 m, at the default 4 cm gate:
      "high": the SLAB_PTS highest points moved up -- z-major stream order puts them LAST (wholly
              rejected chunks among a one-block server's streamed chunks);
      "low":  the SLAB_PTS lowest points moved down -- they sort FIRST (wholly rejected register, LDS
              and streamed chunks).
    A partly filled chunk sits at the seam of both.  (A plain 0.5 m shift, as split_source makes it, puts
    skin points under the boss's cap, 0.5 m above the skin: the gate accepts 28 of them.  Clear of the
    scan's own z range nothing of the CAD is within reach.)  The target is dense (100 000 CAD points: a
    point on the surface misses every one of them within 4 cm with probability
    exp(-pi 0.04^2 1e5 / 17 m^2) ~ 1e-13), so the gate accepts every point left in place; the CPU
    module checks that it rejects exactly the slab."""
    scan, cad, Ttrue = _slab_clouds()
    s = scan.copy()
    by_z = np.argsort(s[:, 2], kind="stable")
    moved = np.zeros(len(s), bool)
    zmin, zmax = s[:, 2].min(), s[:, 2].max()
    if which == "high":
        moved[by_z[-SLAB_PTS:]] = True
        s[moved, 2] += np.float32(SLAB_SHIFT + float(zmax - s[moved, 2].min()))
    elif which == "low":
        moved[by_z[:SLAB_PTS]] = True
        s[moved, 2] -= np.float32(SLAB_SHIFT + float(s[moved, 2].max() - zmin))
    else:
        raise ValueError(which)
    # index order = z order, so the slab is a run of the source's own indices as well
    by_z = np.argsort(s[:, 2], kind="stable")
    return np.ascontiguousarray(s[by_z]), cad, Ttrue, SLAB_GATE, moved[by_z]


SLABS = ("high", "low")


def pair(name, ns=None):
    """(source, target, Ttrue, gate) of "full" (at ns) or a slab"""
    return full_pair(ns) if name == "full" else slab_pair(name)[:4]


def knn_k(ns: int) -> int:
    """k of the covariances: PCL's 20, fewer for a source with fewer points (PCL refuses k > n)"""
    return min(20, ns)


def sweep_transform(Ttrue) -> np.ndarray:
    return np.linalg.inv(Ttrue).astype(np.float32)


def chunk_fill(tgt_index, order) -> list:
    """accepted correspondences per chunk of the stream order `order` (source indices), from the
    oracle's matches (tgt_index[i] < 0: rejected)"""
    ok = np.asarray(tgt_index)[np.asarray(order, np.int64)] >= 0
    return [int(ok[c:c + CHUNK_PTS].sum()) for c in range(0, len(ok), CHUNK_PTS)]


# ---------------------------------------------------------------------------------- oracles
_ORACLES = {}


def oracle(name: str, ns=None):
    """The pair's oracle after its sweep at inv(Ttrue), with the Mahalanobis matrix's upper triangle
    mirrored as the engine stores it (set BEFORE the sweep: it acts there) and the default sum order:
    (oracle, accepted count, target index per source point).  One RefGICP object per pair and k is given
    each source in turn (its target covariances are computed once); the sum order is the caller's to
    set.  A caller that aligns on the oracle calls oracle_stale afterwards (an align sweeps again)."""
    from oracle import ref

    src, tgt, Ttrue, gate = pair(name, ns)
    key = (name, knn_k(len(src)))
    ent = _ORACLES.get(key)
    if ent is None:
        o = ref.RefGICP(max_corr_dist=gate, k=key[1])
        o.set_target(tgt)
        o.set_mahalanobis_upper(True)
        ent = _ORACLES[key] = [o, None]
    o, cur = ent
    if cur is None or cur[0] != len(src):
        assert o.set_source(src) == 0
        m, tj, _, _ = o.correspondences(sweep_transform(Ttrue))
        ent[1] = cur = (len(src), m, tj)
    else:
        o.set_sum_order(0)
    return o, cur[1], cur[2]


def oracle_stale(name: str, ns=None):
    """forget the cached sweep of the pair's oracle (after an align on it)"""
    n = len(pair(name, ns)[0])
    ent = _ORACLES.get((name, knn_k(n)))
    if ent:
        ent[1] = None
