"""Normal clustering (mgicp_normal_clusters, InitialAlignment::obtainNormalsCluster) and the dominant normals
(mgicp_dominant_normals): a NumPy / scipy reference and the cases of test_normal_cluster_inputs.py (CPU) and
test_normal_cluster_gpu.py.

The reference restates the header's rule as PCL runs it: serial rounds in ascending seed; a round is a
breadth-first search from its seed through records that are unprocessed and compatible with the SEED's normal.
Candidate pairs come from a cKDTree over the float64 copies of the float32 coordinates at a radius 1 % above
the tolerance; the link (FLANN's float32 d2 < float32(tol^2)) and the float32 dot are then restated with every
rounding written out.  While it runs it notes how close any decision came to its threshold, in float32 steps:
test_normal_cluster_inputs.py requires every decision to be firm.

Two choices the cases make where a literal reading would put a decision on its threshold:
  * the turning lines turn 4.75 degrees per step, not 5: at 5 the fifth normal lies at eps_angle itself and
    the decision would hang on the last bit of a float dot;
  * the 1 mm planes do put pairs at the tolerance itself (offsets (30, 40), (14, 48), (0, 50) mm and their
    mirrors).  These are the deliberately placed pairs: both sides evaluate the same IEEE expression on the same
    floats, and the inputs test checks that no other pair of these cases comes near.
"""
import math
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree

F32 = np.float32
TOL = float(F32(0.05))               # the reference's tolerance, a float
EPS = 20 * (math.pi / 180.0)         # the reference's eps_angle


# ---- the float32 arithmetic, every rounding written out ---------------------------------------------------
def d2_float(a, b):
    """FLANN's L2_Simple over 3 floats: ((dx^2 + dy^2) + dz^2), each operation rounded to float32"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    d = (a - b).astype(F32)
    sq = (d * d).astype(F32)
    return ((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32)


def dot_float(s, m):
    """PCL's dot of two normals: float products, ((x x' + y y') + z z') rounded to float32 at every step"""
    s, m = np.asarray(s, F32), np.asarray(m, F32)
    p = (s * m).astype(F32)
    return ((p[..., 0] + p[..., 1]).astype(F32) + p[..., 2]).astype(F32)


def c_min(eps_angle):
    """the smallest float32 f with acos((double)f) < eps_angle by libm; +inf when nothing is compatible, -1 above pi"""
    if not eps_angle > 0:
        return F32(np.inf)
    if eps_angle > math.pi:
        return F32(-1.0)
    f = F32(min(1.0, max(-1.0, float(F32(math.cos(eps_angle))))))
    while f > F32(-1.0) and math.acos(float(np.nextafter(f, F32(-2.0)))) < eps_angle:
        f = np.nextafter(f, F32(-2.0))
    while f <= F32(1.0) and not math.acos(float(f)) < eps_angle:
        f = np.nextafter(f, F32(2.0))
    return F32(f)


def _ordered(x):
    """float32 -> integers that order as the floats do (steps between two floats = their difference)"""
    b = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def steps(a, b):
    """|a - b| in float32 steps (NaN: far)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    out = np.abs(_ordered(a) - _ordered(b))
    return np.where(np.isnan(a) | np.isnan(b), np.int64(1) << 40, out)


# ---- the reference ------------------------------------------------------------------------------------------
def reference(xyz, normals, tol=TOL, eps_angle=EPS, min_size=1, max_size=0):
    """-> SimpleNamespace(labels, indices, offsets, clusters, n_rounds, dot_steps, d2_steps, near_pairs):
    dot_steps / d2_steps are the smallest distances, in float32 steps, of any dot from c_min and of any
    candidate pair's d2 from float32(tol^2); near_pairs lists the pairs within 4 steps."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, F32).reshape(-1, 3)
    n = len(xyz)
    r2 = F32(tol * tol)
    cm = c_min(eps_angle)
    finite = np.isfinite(xyz).all(axis=1)
    fidx = np.flatnonzero(finite)
    tree = cKDTree(xyz[fidx].astype(np.float64)) if len(fidx) and r2 > 0 else None
    processed = ~finite
    rounds = []
    dot_steps = d2_steps = np.int64(1) << 40
    near_pairs = []
    for s in range(n):
        if processed[s]:
            continue
        start = processed.copy()  # the state at the start of the round
        members = [s]
        processed[s] = True
        queue = [s]
        while queue:
            nxt = []
            for p in queue:
                if tree is None:
                    continue
                cand = fidx[np.asarray(tree.query_ball_point(xyz[p].astype(np.float64), tol * 1.01), np.int64)]
                cand = cand[cand != p]
                if not len(cand):
                    continue
                d2 = d2_float(xyz[p], xyz[cand])
                st = steps(d2, r2)
                d2_steps = min(d2_steps, st.min())
                near_pairs += [(p, int(j)) for j in cand[st <= 4]]
                linked = cand[d2 < r2]
                linked = linked[~start[linked]]
                if not len(linked):
                    continue
                d = dot_float(normals[s], normals[linked])
                dot_steps = min(dot_steps, steps(d, cm).min())
                ok = (d >= cm) & (d <= F32(1.0))
                for j in linked[ok]:
                    if not processed[j]:
                        processed[j] = True
                        members.append(int(j))
                        nxt.append(int(j))
            queue = nxt
        rounds.append(np.sort(np.asarray(members, np.int32)))
    lo, hi = max(int(min_size), 1), (int(max_size) if max_size else 1 << 62)
    clusters = [m for m in rounds if lo <= len(m) <= hi]
    labels = np.full(n, -1, np.int32)
    for c, m in enumerate(clusters):
        labels[m] = c
    indices = np.concatenate(clusters).astype(np.int32) if clusters else np.zeros(0, np.int32)
    offsets = np.zeros(len(clusters) + 1, np.int64)
    offsets[1:] = np.cumsum([len(m) for m in clusters])
    return SimpleNamespace(labels=labels, indices=indices, offsets=offsets, clusters=clusters, n_rounds=len(rounds),
                           rounds=rounds, dot_steps=int(dot_steps), d2_steps=int(d2_steps), near_pairs=near_pairs)


# ---- the cases ------------------------------------------------------------------------------------------------
def _tilted(deg):
    """unit normals in the x-z plane at `deg` degrees from +z, rounded to float32"""
    a = np.radians(np.asarray(deg, np.float64))
    return np.stack([np.sin(a), np.zeros_like(a), np.cos(a)], axis=-1).astype(F32)


def find_unit_vector(want_above_one, seed=5):
    """a float-normalised unit vector whose float32 self-dot is 1.0000001 (want_above_one) or <= 1, by search"""
    rng = np.random.default_rng(seed)
    for _ in range(10000):
        v = rng.standard_normal(3)
        v = (v / np.linalg.norm(v)).astype(F32)
        if (dot_float(v, v) > F32(1.0)) == want_above_one:
            return v
    raise AssertionError("no such vector found")


def _case(xyz, normals, tol=TOL, eps_angle=EPS, min_size=1, max_size=0, limits=(0, 1), **extra):
    return SimpleNamespace(xyz=np.ascontiguousarray(xyz, F32), normals=np.ascontiguousarray(normals, F32), tol=tol,
                           eps_angle=eps_angle, min_size=min_size, max_size=max_size, limits=tuple(limits),
                           threshold_case=False, placed_pairs=False, **extra)


LINE_TURN = 4.75  # degrees per step (module docstring)


def _turning_line(zero_at):
    """40 points along x at 0.6 tol whose normals turn LINE_TURN per step; index 0 sits at position zero_at,
    the other indices fill the remaining positions in order"""
    pos = np.array([zero_at] + [p for p in range(40) if p != zero_at])
    xyz = np.zeros((40, 3), F32)
    xyz[:, 0] = (pos * (0.6 * TOL)).astype(F32)
    return _case(xyz, _tilted(pos * LINE_TURN), pos=pos)


def _bridge():
    """record 0 (0 degrees) sits above a bridge of two records (15 degrees) and takes it; the sides (30 degrees)
    are compatible with the bridge but more than tol apart without it"""
    s = 0.6 * TOL
    xyz = [(3 * s, s, 0)] + [(3 * s, 0, 0), (4 * s, 0, 0)] + [(k * s, 0, 0) for k in (0, 1, 2)] + [(k * s, 0, 0) for k in (5, 6, 7)]
    return _case(np.array(xyz), _tilted([0, 15, 15, 30, 30, 30, 30, 30, 30]))


def _dropped():
    """{0, 5} is below min_size 3 and record 5 is compatible with the cluster seeded at 1"""
    s = 0.6 * TOL
    order = [0, 5, 1, 2, 3, 4, 6, 7, 8, 9]  # positions along the line
    xyz = np.zeros((10, 3), F32)
    xyz[order, 0] = (np.arange(10) * s).astype(F32)
    deg = np.full(10, 30.0)
    deg[0], deg[5] = 0.0, 15.0
    return _case(xyz, _tilted(deg), min_size=3)


def _patch(above_one):
    g = np.arange(10) * (0.3 * TOL)
    xyz = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    return _case(xyz, np.tile(find_unit_vector(above_one), (100, 1)))


def _threshold(eps_angle):
    """seed normal (0, 0, 1): the float dot with (x, 0, z) is z itself"""
    cm = c_min(EPS)
    zs = np.array([1.0, cm, np.nextafter(cm, F32(-2.0)), 1.0, -1.0], F32)
    nrm = np.stack([np.sqrt(np.maximum(0.0, 1.0 - zs.astype(np.float64) ** 2)), np.zeros(5), zs], axis=-1).astype(F32)
    nrm[:, 2] = zs
    s = 0.3 * TOL
    xyz = np.array([(0, 0, 0), (s, 0, 0), (-s, 0, 0), (0, s, 0), (0, -s, 0)])
    c = _case(xyz, nrm, eps_angle=eps_angle)
    c.threshold_case = True
    return c


def _odd_records():
    """a seed with a NaN normal, a zero normal, a non-finite record and an exact duplicate pair"""
    xyz = np.array([(0, 0, 0), (0.4 * TOL, 0, 0), (np.nan, 0, 0), (0.8 * TOL, 0, 0), (0.8 * TOL, 0, 0), (1.2 * TOL, 0, 0)], F32)
    nrm = np.array([(np.nan, 0, 1), (0, 0, 0), (0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 1)], F32)
    return _case(xyz, nrm)


def _long_line():
    xyz = np.zeros((300, 3), F32)
    xyz[:, 0] = (np.arange(300) * (0.9 * TOL)).astype(F32)
    return _case(xyz, np.tile(F32([0, 0, 1]), (300, 1)), limits=(0, 1, 299, 300, 301))


def _plane(x0=0.0):
    g = np.arange(60) * 0.001
    xyz = np.stack(np.meshgrid(g + x0, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    c = _case(xyz, np.tile(F32([0, 0, 1]), (3600, 1)), limits=(0, 1, 3599, 3600, 3601))
    c.placed_pairs = True
    return c


def _blob():
    """4200 records inside a cube of 0.3 tol: the seed's level claims 4199 at once, more than the 4096 entries
    of the one-workgroup path's LDS frontier, so at a limit of 4096 the entries past it exist only in the spilled
    frontier the level-synchronous path continues from"""
    rng = np.random.default_rng(3)
    xyz = (rng.random((4200, 3)) * (0.3 * TOL)).astype(F32)
    return _case(xyz, np.tile(F32([0, 0, 1]), (4200, 1)), limits=(0, 1, 4096))


CORNERS = (np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) / math.sqrt(3.0)).astype(F32)


def _lattice():
    """16^3 at 0.9 tol; the normal is the cube corner of the coordinates' parities, so no linked pair (one step
    along an axis) shares a direction, and two corners are at least 70 degrees apart"""
    i = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    par = (i % 2) @ np.array([4, 2, 1])
    return _case(i * (0.9 * TOL), CORNERS[par])


_BUILDERS = {
    "line_end": lambda: _turning_line(0),
    "line_middle": lambda: _turning_line(20),
    "bridge": _bridge,
    "dropped": _dropped,
    "patch_above_one": lambda: _patch(True),
    "patch_unit": lambda: _patch(False),
    "threshold_20deg": lambda: _threshold(EPS),
    "threshold_eps_0": lambda: _threshold(0.0),
    "threshold_eps_4": lambda: _threshold(4.0),
    "odd_records": _odd_records,
    "long_line": _long_line,
    "plane": _plane,
    "lattice": _lattice,
    "blob": _blob,
    "far_plane": lambda: _plane(4096.5),
}
CASES = tuple(_BUILDERS)
_CASES, _REFS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def case_reference(name):
    """the case's reference, computed once and shared"""
    if name not in _REFS:
        c = case(name)
        _REFS[name] = reference(c.xyz, c.normals, c.tol, c.eps_angle, c.min_size, c.max_size)
    return _REFS[name]


# ---- dominant normals: the header's tree, restated in float64 ---------------------------------------------------
def _block_tree(v):
    """256 doubles: a wave adds lanes (l, l + d) for d = 32 .. 1, the block its four waves in order"""
    w = np.array(v, np.float64).reshape(4, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w[:, :d] = w[:, :d] + w[:, d:2 * d]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def tree_sum(v):
    """the "Model" rule's fixed tree over the entries v: blocks of 256 (missing entries +0.0), block b's sum
    added to accumulator b % 256 in ascending b, the accumulators through the same tree"""
    v = np.asarray(v, np.float64)
    nb = max(1, -(-len(v) // 256))
    pad = np.zeros(nb * 256)
    pad[:len(v)] = v
    acc = np.zeros(256)
    for b in range(nb):
        acc[b % 256] = acc[b % 256] + _block_tree(pad[256 * b:256 * (b + 1)])
    return _block_tree(acc)


def dominant_reference(normals, clusters, first_twice=True):
    """-> (float32 [len(clusters), 3], float64 sums): the entries are the first member, then every member"""
    normals = np.asarray(normals, F32)[:, :3].astype(np.float64)
    out = np.zeros((len(clusters), 3), F32)
    sums = np.zeros((len(clusters), 3))
    for c, m in enumerate(clusters):
        m = np.asarray(m)
        entries = np.concatenate([m[:1], m]) if first_twice else m
        s = np.array([tree_sum(normals[entries, r]) for r in range(3)])
        z2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        sums[c] = s
        out[c] = (s / np.sqrt(z2) if z2 > 0 else s).astype(F32)
    return out, sums


DOMINANT_SIZES = (1, 2, 3, 64, 65, 257, 70000)


def dominant_case(seed=11):
    """random unit normals and clusters of DOMINANT_SIZES members drawn without order"""
    rng = np.random.default_rng(seed)
    n = 70000
    v = rng.standard_normal((n, 3))
    v[:, 2] = np.abs(v[:, 2]) + 0.5  # a hemisphere: no sum cancels
    normals = (v / np.linalg.norm(v, axis=1)[:, None]).astype(F32)
    clusters = [rng.permutation(n)[:k].astype(np.int32) for k in DOMINANT_SIZES]
    return normals, clusters
