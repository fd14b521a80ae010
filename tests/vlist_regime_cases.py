"""Clouds, transforms and NumPy premises of the 1-NN cell-list regime tests.

Shared by tests/test_vlist_regime_inputs.py (CPU: the premises that do not depend on the engine's grid)
and tests/test_vlist_regime_gpu.py (engine vs oracle vs the engine without lists, and the regime
certification from GICPEngine.vlist_layout).  Nothing here touches the engine.  Every builder is cached:
a cloud is made once per process and must not be modified.

The regimes are those of vl_build_cell and its callers (csrc/mgicp_kernels.hip, DESIGN.md "1-NN cell
lists"): long lists (count field 63, true count in a header entry), the build's second pass (513..1024
candidates), its slot scan (no room at the free end of the build list), candidate overflow (more than
1024), a full pool, the grown fine cell and lists switched off (wide gates), and queries anywhere in a
cell's box, not only on the target's surface.
"""
import functools

import numpy as np

GATE = 0.04            # GICPAlignment's max correspondence distance
CAND_FIRST = 512       # kVlCandS: candidates the build's first pass keeps
CAND_MAX = 1024        # kVlCand: candidates the second pass keeps; more: an overflow cell
LONG = 63              # kVlLong: lists of this many entries or more carry a header
PAIR_MAX = 256         # survivors stage 2 tests against each other; more are kept as they are
PITCH = 0.005
SHEET_N = 64
ORIGIN = np.array([1.0, 2.0, 0.5])
P_OFF = 0.2            # the copies / the clump sit this far off the sheet
BALL_R, SHELL_R = 0.03, (0.035, 0.045)
CORE_R = 0.0003        # extra ball queries right at P: the cells that hold the clump's points
CLUMP_R = 0.0002
PCL_DEFAULT_GATE = float(np.sqrt(np.finfo(np.float64).max))  # Registration::corr_dist_threshold_

STATES = ("not_built", "touched", "requested", "reject", "overflow", "listed")
NOT_BUILT, TOUCHED, REQUESTED, REJECT, OVERFLOW, LISTED = range(6)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@functools.lru_cache(maxsize=None)
def sheet() -> np.ndarray:
    """a jittered 64 x 64 sheet at 5 mm pitch (jitter +-1 mm in the plane, +-0.5 mm off it)"""
    g = _rng(11)
    i, j = np.meshgrid(np.arange(SHEET_N), np.arange(SHEET_N), indexing="ij")
    p = np.stack([i.ravel() * PITCH, j.ravel() * PITCH, np.zeros(SHEET_N * SHEET_N)], 1)
    p += g.uniform(-1.0, 1.0, p.shape) * np.array([1e-3, 1e-3, 5e-4])
    out = np.ascontiguousarray(p + ORIGIN, np.float32)
    out.setflags(write=False)
    return out


def point_p() -> np.ndarray:
    """P: above the middle of the sheet, 0.2 m off it"""
    mid = (SHEET_N - 1) * PITCH / 2
    return (ORIGIN + np.array([mid + 0.0007, mid - 0.0011, P_OFF])).astype(np.float32)


def _ball(g, n, r0, r1):
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.cbrt(g.uniform(r0 ** 3, r1 ** 3, size=(n, 1)))
    return d * r


@functools.lru_cache(maxsize=None)
def probe_source():
    """(source, roles): the queries of the dup / clump cases.  roles: 0 ball (2000 uniform within 0.03 m
    of P, and 300 within 0.3 mm of it), 1 shell (500 at 0.035..0.045 m, either side of the gate), 2 the
    sheet shifted by 2 mm."""
    g = _rng(12)
    P = point_p().astype(np.float64)
    ball = P + _ball(g, 2000, 0.0, BALL_R)
    core = P + _ball(g, 300, 0.0, CORE_R)
    shell = P + _ball(g, 500, *SHELL_R)
    sh = sheet().astype(np.float64) + np.array([0.0012, -0.0011, 0.0012])  # |shift| = 2.02 mm
    src = np.ascontiguousarray(np.concatenate([ball, core, shell, sh]), np.float32)
    roles = np.concatenate([np.zeros(2300, np.int8), np.ones(500, np.int8), np.full(len(sh), 2, np.int8)])
    src.setflags(write=False)
    roles.setflags(write=False)
    return src, roles


@functools.lru_cache(maxsize=None)
def dup_target(n: int) -> np.ndarray:
    """the sheet plus n exact copies of P, appended last (the oracle's winner: their lowest index)"""
    out = np.ascontiguousarray(np.concatenate([sheet(), np.repeat(point_p()[None], n, 0)]), np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def clump_target(n: int) -> np.ndarray:
    """the sheet plus n distinct points in the ball of radius 0.2 mm about P, appended last"""
    g = _rng(100 + n)
    pts = (point_p().astype(np.float64) + _ball(g, n, 0.0, CLUMP_R)).astype(np.float32)
    out = np.ascontiguousarray(np.concatenate([sheet(), pts]), np.float32)
    out.setflags(write=False)
    return out


def probe_transforms():
    """identity and a small shift (new cells near P, the shell still either side of the gate)"""
    I = np.eye(4, dtype=np.float32)
    S = np.eye(4, dtype=np.float32)
    S[:3, 3] = [0.0031, -0.0017, 0.0023]
    return [I, S]


@functools.lru_cache(maxsize=None)
def part():
    """(scan, cad, T_true) of the synthetic 20k / 20k part"""
    from leica_point_cloud_processing_amd import synth

    scan, cad, T = synth.scan_vs_cad(20000, 20000)
    for a in (scan, cad):
        a.setflags(write=False)
    return scan, cad, T


@functools.lru_cache(maxsize=None)
def cluttered_scan() -> np.ndarray:
    """the same part scanned with 4 % clutter 5..30 cm off the surface and 400 debris points: a scan-like
    source (GICP converges) whose clutter queries fall in off-surface cells"""
    from leica_point_cloud_processing_amd import synth

    scan, cad, T = synth.scan_vs_cad(20000, 20000, clutter=0.04, debris=400)
    assert np.array_equal(cad, part()[1])
    scan.setflags(write=False)
    return scan


# 0.04, 0.10, 0.15: no cell of the 20k part gathers more than 512 candidates (the candidate radius is at
# most the cell's distance to the surface plus its diagonal, and the part has ~28 mm between neighbours),
# nor does any gate up to 0.6 m; 0.7 m reaches the second pass with one cell, 0.8 m with none, 0.9 m and
# every larger gate probed (1.0 .. 3.0) with 9 or more: VOLUME_RAISED.  Candidate overflow starts at 2.5 m
# (7 cells; none at 2.0): VOLUME_OVERFLOW.
VOLUME_RAISED, VOLUME_OVERFLOW = 0.9, 2.5
VOLUME_GATES = (0.04, 0.10, 0.15, VOLUME_RAISED, VOLUME_OVERFLOW)


@functools.lru_cache(maxsize=None)
def volume_source(gate: float) -> np.ndarray:
    """20k points uniform in the target's bbox grown by the gate: off-surface queries, where the
    candidate radius is the gate itself and the lists are as long as they get"""
    cad = part()[1].astype(np.float64)
    lo, hi = cad.min(0) - gate, cad.max(0) + gate
    g = _rng(200 + int(round(gate * 1000)))
    out = np.ascontiguousarray(g.uniform(lo, hi, size=(20000, 3)), np.float32)
    out.setflags(write=False)
    return out


def xform32(T, pts) -> np.ndarray:
    """Eigen's Matrix4f * Vector4f in fp32, as the sweeps compute a query: ((c0 x + c1 y) + c2 z) + c3"""
    T = np.asarray(T, np.float32)
    p = np.asarray(pts, np.float32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return ((T[None, :3, 0] * x + T[None, :3, 1] * y) + T[None, :3, 2] * z) + T[None, :3, 3]


def cell_index(lay, q):
    """fp64 fine cell of every query from a layout (GICPEngine.vlist_layout): (ci, inside, near) -- the
    cell index, whether it lies in the grid, and whether the query is within es of a cell face (its fp32
    assignment may then differ: such queries are left out of a regime's count)"""
    g = (np.asarray(q, np.float64) - np.array([lay["ox"], lay["oy"], lay["oz"]])) / lay["c"]
    i = np.floor(g)
    near = (np.minimum(g - i, i + 1.0 - g) * lay["c"] <= lay["es"]).any(1)
    n = np.array([lay["nx"], lay["ny"], lay["nz"]])
    inside = ((i >= 0) & (i < n)).all(1)
    ii = np.where(inside[:, None], i, 0).astype(np.int64)
    return ii[:, 0] + n[0] * (ii[:, 1] + n[1] * ii[:, 2]), inside, near


def cell_index_f32(lay, q):
    """the sweeps' own fp32 assignment floor((q - o) * inv_c) (qcell): (ci, inside)"""
    q = np.asarray(q, np.float32)
    o = np.array([lay["ox"], lay["oy"], lay["oz"]], np.float32)
    f = np.floor((q - o) * np.float32(lay["inv_c"]))
    n = np.array([lay["nx"], lay["ny"], lay["nz"]])
    inside = ((f >= 0) & (f < n)).all(1)
    ii = np.where(inside[:, None], f, 0).astype(np.int64)
    return ii[:, 0] + n[0] * (ii[:, 1] + n[1] * ii[:, 2]), inside


def near_face_share(q, o, c, es) -> float:
    """share of the queries within es of a face of a grid of edge c at origin o (fp64)"""
    g = (np.asarray(q, np.float64) - np.asarray(o, np.float64)) / c
    i = np.floor(g)
    return float((np.minimum(g - i, i + 1.0 - g) * c <= es).any(1).mean())


def es_of(target, gate, c) -> float:
    """vl_prepare's es for a target, a gate and a cell edge"""
    t = np.asarray(target, np.float64)
    pad = gate * (1.0 + 1e-5) + 1e-9 + 2.0 * c
    return 3.0e-6 * (np.abs(t).max() + pad + (t.max(0) - t.min(0)).max()) + 1e-4 * c


def padded(length):
    """pool entries a list of that true length occupies: a multiple of 4, + 4 for a long list's header"""
    length = np.asarray(length, np.int64)
    return ((length + 3) & ~3) + np.where(length >= LONG, 4, 0)


def pool_ranges_ok(state, length, offset, pool_cap):
    """(inside, disjoint): every listed cell's padded range [off, off + cnt4) lies inside the pool, and
    no two ranges overlap (sorted by offset: each ends at or before the next one's start)"""
    m = state == LISTED
    off = offset[m].astype(np.int64)
    end = off + padded(length[m])
    o = np.argsort(off, kind="stable")
    off, end = off[o], end[o]
    inside = bool((end <= pool_cap).all())
    disjoint = bool((end[:-1] <= off[1:]).all())
    return inside, disjoint


def corner_queries(lay, cells) -> np.ndarray:
    """queries probing the whole box of each given fine cell: its 8 corners, 6 face centres and centre,
    each corner nudged one float step inwards and one outwards, and points es / 2 outside each face"""
    nx, ny = lay["nx"], lay["ny"]
    cells = np.asarray(cells, np.int64)
    idx = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1).astype(np.float64)
    o = np.array([lay["ox"], lay["oy"], lay["oz"]])
    c, es = lay["c"], lay["es"]
    lo = o + idx * c
    out = []
    corners = np.array([[(k >> d) & 1 for d in range(3)] for k in range(8)], np.float64)
    for k in corners:
        p = (lo + k * c).astype(np.float32)
        inward = np.where(k > 0, -np.inf, np.inf).astype(np.float32)
        out += [p, np.nextafter(p, inward[None]), np.nextafter(p, -inward[None])]
    for d in range(3):
        for side in (0.0, 1.0):
            f = np.full(3, 0.5)
            f[d] = side
            out.append((lo + f * c).astype(np.float32))
            g = f.copy()
            g[d] = side + (0.5 * es / c) * (1 if side else -1)
            out.append((lo + g * c).astype(np.float32))
    out.append((lo + 0.5 * c).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(out), np.float32)
