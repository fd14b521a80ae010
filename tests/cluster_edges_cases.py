"""Clouds and references of the clustering / voxel-grid edge tests.

Shared by tests/test_cluster_edges_inputs.py (CPU: every cloud is what it claims to be, the references
agree with brute force on it) and tests/test_cluster_edges_gpu.py (engine vs reference), and by
tests/test_euclidean_clusters.py, whose reference helpers live here.  Nothing in this module touches
the engine.  Every builder is cached: a cloud is made once per process and must not be modified.

Expected results come from `ref_clusters` / `bruteforce_clusters` (the fp32 FLANN predicate in numpy)
alone.  `grid_of` restates the engine's cell index in float32 numpy ONLY to select inputs and to
certify that an input reaches a regime (cells three apart, one populous cell, no same-cell shortcut);
it never produces an expected clustering.
"""
import functools

import numpy as np

F32 = np.float32
INF32 = F32(np.inf)
TINY32 = F32(1.17549435e-38)  # the smallest normal float
MAX_CELLS = 1 << 29            # the dense cell table's cap (kMaxCells)
SHORTCUT_MAX_DIM = 1 << 18     # kCcShortcutMaxDim
REACH = 3                      # kCcReach
BOX_MIN_PAIRS = 4096           # kCcBoxMinPairs


# ---------------------------------------------------------------------------------------
# the test-side reference
# ---------------------------------------------------------------------------------------
def d2_f32(a, b):
    """FLANN L2_Simple in fp32, one rounding per operation: ((dx*dx) + dy*dy) + dz*dz."""
    with np.errstate(over="ignore", under="ignore"):  # +inf and denormals are results like any other here
        d = (a.astype(np.float32) - b.astype(np.float32)).astype(np.float32)
        d2 = ((d[..., 0] * d[..., 0]).astype(np.float32) + (d[..., 1] * d[..., 1]).astype(np.float32)).astype(np.float32)
        return (d2 + (d[..., 2] * d[..., 2]).astype(np.float32)).astype(np.float32)


def r2_of(tol):
    """FLANN's radius: float(tolerance^2); 0, denormal or +inf at the ends of the range"""
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(np.float64(tol) * np.float64(tol))


def finish(xyz, fin_idx, comp, min_size, max_size):
    """components (label per finite point) -> (clusters, labels, offsets, n_components) by the rule."""
    n = len(xyz)
    order = np.argsort(comp, kind="stable")  # members ascending inside a component
    bounds = np.flatnonzero(np.diff(comp[order])) + 1
    groups = [fin_idx[g] for g in np.split(order, bounds)] if len(order) else []
    lo, hi = max(int(min_size), 1), (int(max_size) if max_size else np.iinfo(np.int64).max)
    kept = [g for g in groups if lo <= len(g) <= hi]
    kept.sort(key=lambda g: (-len(g), int(g[0])))
    labels = np.full(n, -1, np.int32)
    for c, g in enumerate(kept):
        labels[g] = c
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in kept])]).astype(np.int64)
    return [g.astype(np.int32) for g in kept], labels, offsets, len(groups)


def components(xyz, tol):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin_idx = np.flatnonzero(np.isfinite(xyz).all(1))
    pts = xyz[fin_idx]
    m = len(pts)
    r2 = r2_of(tol)
    i = j = np.zeros(0, np.int64)
    if m > 1 and r2 > 0:
        # every pair the fp32 predicate accepts has an exact distance below tol (1 + 1e-6)
        cand = cKDTree(pts.astype(np.float64)).query_pairs(float(tol) * (1 + 1e-5) + 1e-30, output_type="ndarray")
        if len(cand):
            ok = d2_f32(pts[cand[:, 0]], pts[cand[:, 1]]) < r2
            i, j = cand[ok, 0], cand[ok, 1]
    if m == 0:
        return fin_idx, np.zeros(0, np.int64)
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(m, m))
    _, comp = connected_components(g, directed=False)
    return fin_idx, comp.astype(np.int64)


def ref_clusters(xyz, tol, min_size=1, max_size=0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin_idx, comp = components(xyz, tol)
    return finish(xyz, fin_idx, comp, min_size, max_size)


def bruteforce_clusters(xyz, tol, min_size=1, max_size=0):
    """All pairs, own union-find: independent of the kd-tree candidates and of csgraph."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin_idx = np.flatnonzero(np.isfinite(xyz).all(1))
    pts = xyz[fin_idx]
    m = len(pts)
    adj = d2_f32(pts[:, None, :], pts[None, :, :]) < r2_of(tol)
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(*np.nonzero(np.triu(adj, 1))):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    comp = np.array([find(x) for x in range(m)], np.int64)
    return finish(xyz, fin_idx, comp, min_size, max_size)


def same_result(a, b):
    """two (clusters, labels, offsets, n_components) results are identical"""
    ac, al, ao, an = a
    bc, bl, bo, bn = b
    return (an == bn and len(ac) == len(bc) and all(np.array_equal(x, y) for x, y in zip(ac, bc))
            and np.array_equal(al, bl) and np.array_equal(ao, bo))


def fod_cloud(seed=0, n=3000):
    """The FOD scenario of tests/test_fod_filters.py: a synthetic scan plus 4 foreign-object blobs, with
    a NaN record and an Inf record."""
    from leica_point_cloud_processing_amd import synth

    scan, cad, _ = synth.scan_vs_cad(n, 500)
    rng = np.random.default_rng(seed)
    blobs = (cad[rng.integers(0, len(cad), 4)][:, None, :] +
             rng.normal(0, 0.004, (4, 25, 3)) + np.array([0, 0, 0.03])).reshape(-1, 3).astype(np.float32)
    a = np.concatenate([scan, blobs]).astype(np.float32)
    a[7] = np.nan
    a[len(a) - 5, 1] = np.inf
    return a


# ---------------------------------------------------------------------------------------
# the grid's cell index, restated
# ---------------------------------------------------------------------------------------
class Grid:
    """origin o (3 float32), h (float64), inv_h (float32), dims (3 ints), shortcut (bool)"""

    def __init__(self, o, h, inv_h, dims, shortcut):
        self.o, self.h, self.inv_h, self.dims, self.shortcut = o, h, inv_h, dims, shortcut

    def cells(self, xyz):
        """per-axis cell indices (m, 3) int64: clip(floor(fl(fl(v - o) * inv_h)), 0, n - 1)"""
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        f = np.floor(((xyz - self.o).astype(np.float32) * self.inv_h).astype(np.float32))
        return np.clip(f.astype(np.int64), 0, np.asarray(self.dims, np.int64) - 1)

    def keys(self, xyz):
        c = self.cells(xyz)
        return c[:, 0] + self.dims[0] * (c[:, 1] + self.dims[1] * c[:, 2])

    @property
    def table_bytes(self):
        return 4 * (int(np.prod(np.asarray(self.dims, np.int64))) + 1)


def grid_of(xyz, tol):
    """A float32 numpy restatement of the clustering grid (the engine's build_grid with a forced cell
    edge, and the condition of its same-cell shortcut):
      o = the finite points' float32 minimum per axis, ext = float32(max - o),
      h = max(reach / 2, max(ext) / 2^20) with reach = tol (sqrt(float(tol^2)) if that is larger and
      float(tol^2) is denormal), grown further only while the cell table exceeds MAX_CELLS,
      inv_h = float32(1 / h), n = floor(float64(ext) * inv_h) + 1.
    It only SELECTS and CERTIFIES inputs (this pair's computed cells are three apart, this cell holds 130
    points, this grid is past the shortcut's width).  It never produces an expected clustering: those
    come from ref_clusters / bruteforce_clusters, which know nothing of cells."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    pts = xyz[np.isfinite(xyz).all(1)]
    o = pts.min(0)
    ext = (pts.max(0) - o).astype(np.float32)
    r2 = r2_of(tol)
    reach = float(tol)
    if r2 < TINY32:
        reach = max(reach, float(np.sqrt(np.float64(r2))))
    h = max(0.5 * reach, float(ext.max()) / 1048576.0)

    def dims(h):
        inv_h = np.float32(1.0 / h)
        nd = [int(np.floor(float(e) * float(inv_h))) + 1 for e in ext]
        return nd, nd[0] * nd[1] * nd[2]

    nd, nc = dims(h)
    while nc > MAX_CELLS:
        h *= np.cbrt(nc / MAX_CELLS) * 1.01
        nd, nc = dims(h)
    inv_h = np.float32(1.0 / h)
    shortcut = bool(r2 >= TINY32 and np.isfinite(r2) and inv_h == np.float32(1.0 / (0.5 * float(tol)))
                    and max(nd) <= SHORTCUT_MAX_DIM)
    return Grid(o, h, inv_h, nd, shortcut)


def cell_counts(xyz, tol):
    """(grid, sorted unique cell keys, their point counts)"""
    g = grid_of(xyz, tol)
    k, c = np.unique(g.keys(xyz), return_counts=True)
    return g, k, c


def occupied_cells_isolated(xyz, tol):
    """no two occupied cells within the link kernel's reach of each other (Chebyshev distance <= REACH)"""
    g = grid_of(xyz, tol)
    c = np.unique(g.cells(xyz), axis=0)
    d = np.abs(c[:, None, :] - c[None, :, :]).max(-1)
    np.fill_diagonal(d, REACH + 1)
    return bool((d > REACH).all())


def expected_pair_tests(xyz, tol):
    """The link kernel's distance evaluations (info["pair_tests"]) on a cloud whose occupied cells are out
    of each other's reach, derived from the documented behaviour and not measured: none with the same-cell
    shortcut, every pair of every cell without it.  The counts per cell come from the restated cell
    function."""
    g, _, counts = cell_counts(xyz, tol)
    assert occupied_cells_isolated(xyz, tol)
    return 0 if g.shortcut else int(sum(int(n) * (int(n) - 1) // 2 for n in counts))


def last_linked(a, b, tol, ax, towards=+1):
    """b, a point about one tolerance from a, moved along axis `ax` by single float steps (`towards` = +1:
    upwards is away from a) to the LAST float that the fp32 predicate still links to a; returns
    (that b, the first unlinked b one step further).  a and b are 3-vectors."""
    a, b = np.asarray(a, np.float32), np.array(b, np.float32)
    r2 = r2_of(tol)
    step = INF32 if towards > 0 else -INF32
    while d2_f32(a, b) < r2:
        b[ax] = np.nextafter(b[ax], step)
    while not d2_f32(a, b) < r2:
        b[ax] = np.nextafter(b[ax], -step)
    out = b.copy()
    out[ax] = np.nextafter(b[ax], step)
    assert d2_f32(a, b) < r2 and not d2_f32(a, out) < r2
    return b, out


# ---------------------------------------------------------------------------------------
# Family A: linked pairs whose computed cells are three apart
# ---------------------------------------------------------------------------------------
A_TOL = 1.2e-3
A_ORIGIN = -100.37
A_CELLS = (1 << 18) - 8          # the issue's configuration: the grid still takes the same-cell shortcut
A_CELLS_WIDE = (1 << 20) - 8     # the widest grid of tol / 2 cells: no shortcut, the cell index's error largest
A_STRIDE = 24       # candidate cell borders: a pair spans four cells, the next one starts 20 cells on
A_MAX_PAIRS = 200


@functools.lru_cache(maxsize=None)
def _reach_line(n_cells=A_CELLS):
    """The 1-D coordinates of Family A: (values, pair index ranges, twin index ranges).
    Anchors at both ends pin the bounding box: n_cells cells of tol / 2 from an origin far from zero.
    Candidates: a one hundredth of a cell below a cell border, b the largest float with d2(a, b) < r2.
    Where the restated cell indices of a and b are three apart the pair is kept; every second kept pair
    gets a twin at a border whose candidate did not qualify, with b one float step further (not linked)."""
    h = 0.5 * A_TOL
    o = F32(A_ORIGIN)
    end = F32(float(o) + (n_cells - 0.5) * h)
    anchors = np.array([[o, 0, 0], [end, 0, 0]], np.float32)
    g = grid_of(anchors, A_TOL)
    assert g.dims == [n_cells, 1, 1] and g.shortcut == (n_cells <= SHORTCUT_MAX_DIM)
    borders = np.arange(A_STRIDE, n_cells - A_STRIDE - 2, A_STRIDE)
    a = (float(o) + (borders - 0.01) * h).astype(np.float32)
    b = (a.astype(np.float64) + A_TOL).astype(np.float32)
    r2 = r2_of(A_TOL)

    def d2(a, b):
        d = (b - a).astype(np.float32)
        return (d * d).astype(np.float32)

    for _ in range(64):  # vectorised last_linked: b to the last linked float, b1 the first unlinked one
        lk = d2(a, b) < r2
        nb = np.where(lk, np.nextafter(b, INF32), np.nextafter(b, -INF32)).astype(np.float32)
        done = lk & ~(d2(a, nb) < r2)
        if done.all():
            break
        b = np.where(done, b, nb)
    assert done.all()
    b1 = np.nextafter(b, INF32)

    def cell(v):
        return g.cells(np.stack([v, np.zeros_like(v), np.zeros_like(v)], 1))[:, 0]

    three = np.flatnonzero(cell(b) - cell(a) == 3)
    rest = np.flatnonzero(cell(b) - cell(a) != 3)
    three = three[np.linspace(0, len(three) - 1, min(len(three), A_MAX_PAIRS)).astype(np.int64)]  # all along
    twins = rest[np.linspace(0, len(rest) - 1, len(three) // 2).astype(np.int64)]
    vals = np.concatenate([anchors[:, 0], np.stack([a[three], b[three]], 1).ravel(),
                           np.stack([a[twins], b1[twins]], 1).ravel()]).astype(np.float32)
    n_pairs, n_twins = len(three), len(twins)
    pairs = 2 + 2 * np.arange(n_pairs)
    twin_idx = 2 + 2 * n_pairs + 2 * np.arange(n_twins)
    return vals, pairs, twin_idx


@functools.lru_cache(maxsize=None)
def reach_three(axis: int, n_cells: int = A_CELLS):
    """(xyz shuffled, tol, pairs (m, 2) indices of linked pairs three cells apart, twins (k, 2) indices
    of unlinked pairs): the line of Family A along `axis`, the other two coordinates zero"""
    vals, pairs, twins = _reach_line(n_cells)
    xyz = np.zeros((len(vals), 3), np.float32)
    xyz[:, axis] = vals
    perm = np.random.default_rng(100 + axis).permutation(len(vals))
    inv = np.argsort(perm)
    return (np.ascontiguousarray(xyz[perm]), A_TOL, np.stack([inv[pairs], inv[pairs + 1]], 1),
            np.stack([inv[twins], inv[twins + 1]], 1))


# ---------------------------------------------------------------------------------------
# Family B: the box prune at one float step
# ---------------------------------------------------------------------------------------
B_TOL = 0.03
B_NA, B_NB = 130, 70


def _clump_pair(tol, arrangement, mirrored, seed, cell_a, yz_frac):
    """(A (130, 3), B_linked (70, 3), B_apart (70, 3)) in units where cells are tol / 2 wide from 0.
    A's extreme point is its LAST row, B's its row 35.  The clumps face each other along +x (A in cell
    `cell_a`, B two cells further) or, mirrored, along -x (B two cells before A); "corner" offsets them
    the same way on y and z as well.  `yz_frac`: the part of a cell the clumps may use on the axes where
    they overlap (Family C keeps every point in one y / z cell)."""
    rng = np.random.default_rng(seed)
    h = 0.5 * tol
    s = -1.0 if mirrored else 1.0
    axes = (0, 1, 2) if arrangement == "corner" else (0,)
    # extreme points, in cells: A's faces B from fa inside its cell, B's lies `gap` further
    ea = np.empty(3)
    eb = np.empty(3)
    for d in range(3):
        if d in axes:
            ca = cell_a if not mirrored else cell_a + 2
            fa = 0.5 if arrangement == "axis" else 0.93
            ea[d] = ca + (fa if not mirrored else 1.0 - fa)
            gap = 2.0 if arrangement == "axis" else 1.14  # corner: 1.14, 1.14 and the rest on z below
            eb[d] = ea[d] + s * gap
        else:
            ea[d] = eb[d] = 0.5 * yz_frac
    pa = (ea * h).astype(np.float32)
    pb = (eb * h).astype(np.float32)
    if arrangement == "corner":
        dz = np.sqrt(4.0 - 2 * 1.14 ** 2)  # 1.183 cells: |pb - pa| = tol
        pb[2] = F32((ea[2] + s * dz) * h)
    last = 2 if arrangement == "corner" else 0
    pb_in, pb_out = last_linked(pa, pb, tol, last, towards=+1 if s > 0 else -1)
    # the other points: behind their extreme point on the facing axes, anywhere on the overlapping ones
    def rest(n, e_pt, e_cells, sign, beyond):
        p = np.empty((n, 3), np.float32)
        for d in range(3):
            if d in axes:
                c = np.floor(e_cells[d])
                lo, hi = (c + 0.03, e_cells[d] - 0.01) if sign > 0 else (e_cells[d] + 0.01, c + 0.97)
                p[:, d] = (rng.uniform(lo, hi, n) * h).astype(np.float32)
                p[:, d] = np.minimum(p[:, d], e_pt[d]) if sign > 0 else np.maximum(p[:, d], beyond[d])
            else:
                p[:, d] = (rng.uniform(0.05, 0.95, n) * yz_frac * h).astype(np.float32)
        return p
    A = np.concatenate([rest(B_NA - 1, pa, ea, s, pa), pa[None]])
    eb_c = pb_out.astype(np.float64) / h
    rb = rest(B_NB - 1, pb_out, eb_c, -s, pb_out)
    B_in = np.concatenate([rb[:35], pb_in[None], rb[35:]])
    B_out = np.concatenate([rb[:35], pb_out[None], rb[35:]])
    return A.astype(np.float32), B_in.astype(np.float32), B_out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def box_prune(arrangement: str, step: str, mirrored: bool):
    """(xyz, tol, index of A's extreme point, index of B's extreme point); rows: the origin point, A's
    130 points (the extreme one last), B's 70 (the extreme one in the middle).  `step`: "linked" (B's
    extreme point is the largest float still linked to A's) or "apart" (one float step further)."""
    A, B_in, B_out = _clump_pair(B_TOL, arrangement, mirrored, seed=21, cell_a=10, yz_frac=1.0)
    if arrangement == "axis":  # overlap on y and z, away from the origin point's cells
        for c in (A, B_in, B_out):
            c[:, 1:] += F32(3 * 0.5 * B_TOL)
        B_in[35, 1:] = B_out[35, 1:] = A[-1, 1:]
    xyz = np.concatenate([np.zeros((1, 3), np.float32), A, B_in if step == "linked" else B_out])
    return np.ascontiguousarray(xyz, np.float32), B_TOL, B_NA, B_NA + 1 + 35


def box_gap_f32(A, B):
    """cc_boxes_apart's G in float32 numpy: the squared gap of the two bounding boxes"""
    G = F32(0)
    for d in range(3):
        g = max(F32(B[:, d].min() - A[:, d].max()), F32(A[:, d].min() - B[:, d].max()), F32(0))
        G = F32(G + F32(g * g))
    return G


# ---------------------------------------------------------------------------------------
# Families C and D: regime switches with small cell tables, populous cells without the shortcut
# ---------------------------------------------------------------------------------------
C_TOL = 1.2e-3
C_H = 0.5 * C_TOL
REGIMES = {  # name -> the x anchor, in cells of tol / 2
    "shortcut": (1 << 18) - 16 - 0.5,
    "wide": (1 << 18) + 16 - 0.5,
    "widest": (1 << 20) - 16 - 0.5,
    "clamped": 1.5 * (1 << 20),
    "clamped3": 3.0 * (1 << 20),  # Family D only: cells of 1.5 tol, about half the pairs of a cell link
    "clamped8": 8.0 * (1 << 20),  # Family D only: cells of 4 tol, the sparser cells fall into several components
}


def _regime_h(regime):
    """the grid's cell edge in the regime (the anchor decides it)"""
    anchor = F32(REGIMES[regime] * C_H)
    return max(C_H, float(anchor) / 1048576.0), anchor


def _cell_points(rng, n, cell, h, lo=0.15, hi=0.85, yz_h=C_H):
    """n points spread inside x cell `cell` of edge h; y and z inside the first tol / 2 cell"""
    p = np.empty((n, 3), np.float64)
    p[:, 0] = (cell + rng.uniform(lo, hi, n)) * h
    p[:, 1:] = rng.uniform(min(lo, 0.05), min(hi, 0.9), (n, 2)) * yz_h
    return p.astype(np.float32)


C_ISOLATED = ((40, 97), (61, 100), (5000, 103), (131071, 100), (200003, 99), (262100, 101))


@functools.lru_cache(maxsize=None)
def regime_witness(regime: str):
    """(xyz, tol): isolated populous cells only (about 100 points each, no neighbour within four cells)
    plus the two anchors.  pair_tests of the link kernel is 0 with the same-cell shortcut and exactly
    the sum of C(n_c, 2) over the cells without it."""
    rng = np.random.default_rng(31)
    h, anchor = _regime_h(regime)
    cells = [_cell_points(rng, n, c, h) for c, n in C_ISOLATED]
    xyz = np.concatenate([np.zeros((1, 3), np.float32), np.array([[anchor, 0, 0]], np.float32)] + cells)
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))], np.float32), C_TOL


@functools.lru_cache(maxsize=None)
def regime_full(regime: str):
    """(xyz, tol): the witness cloud plus Family B's axis-gap clumps at this tolerance, in both steps
    and both cell orders, all inside one y / z cell (the table stays nx x 1 x 1)"""
    w, _ = regime_witness(regime)
    parts = [w]
    k = 0
    for mirrored in (False, True):
        for step in (0, 1):
            A, B_in, B_out = _clump_pair(C_TOL, "axis", mirrored, seed=40 + k, cell_a=1000 + 40 * k, yz_frac=0.9)
            B = B_in if step == 0 else B_out
            B[35, 1:] = A[-1, 1:]
            parts += [A, B]
            k += 1
    return np.ascontiguousarray(np.concatenate(parts), np.float32), C_TOL


@functools.lru_cache(maxsize=None)
def denormal_radius():
    """(xyz, tol = 1e-20): float(tol^2) = 1e-40 is denormal and > 0.  300 base points uniform in
    [0, 1e-18]^3, 100 partners at +0.6e-20 along x (linked), 100 at +1.5e-20 along y (not linked)."""
    rng = np.random.default_rng(7)
    base = rng.uniform(0.0, 1e-18, (300, 3)).astype(np.float32)
    px = base[:100].copy()
    px[:, 0] = (px[:, 0].astype(np.float64) + 0.6e-20).astype(np.float32)
    py = base[100:200].copy()
    py[:, 1] = (py[:, 1].astype(np.float64) + 1.5e-20).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([base, px, py]), np.float32), 1e-20


@functools.lru_cache(maxsize=None)
def infinite_radius():
    """(xyz, tol = 1e20): float(tol^2) overflows to +inf.  Every pair whose float d2 is finite links, a
    pair whose d2 overflows too (inf < inf is false) does not: 60 points within 1e18 of the origin, 40
    within 1e18 of (1.5e19, 0, 0) (d2 ~ 2.3e38, finite: linked to the first group), 30 around
    (-1.5e19, 1.2e19, 0) (linked to the first group, d2 = inf against the second) and one point at 3e19 on
    z, out of every other point's finite range."""
    rng = np.random.default_rng(19)
    parts = [rng.uniform(-1e18, 1e18, (60, 3)),
             rng.uniform(-1e18, 1e18, (40, 3)) + [1.5e19, 0, 0],
             rng.uniform(-1e18, 1e18, (30, 3)) + [-1.5e19, 1.2e19, 0],
             np.array([[0, 0, 3e19]])]
    xyz = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))]), 1e20


D_SIZES = (1, 2, 63, 64, 65, 129, 200)
D_NEIGHBOURS = ((1, 200), (200, 1), (64, 65), (65, 64))


@functools.lru_cache(maxsize=None)
def populous_cells(regime: str):
    """(xyz, tol, {x cell: points}): isolated cells of D_SIZES points and neighbouring pairs of cells in
    both size orders, on a grid without the same-cell shortcut.  "wide": cells of tol / 2 -- every pair
    of ONE such cell links whatever the spacing (the shortcut's own premise), the mixed outcomes are those
    of the neighbouring cells' pairs; "clamped3": cells of 1.5 tol filled edge to edge, about half the
    pairs of one cell link; "clamped8": cells of 4 tol, the sparser cells fall into several components."""
    rng = np.random.default_rng(53)
    h, anchor = _regime_h(regime)
    lo, hi = (0.15, 0.85) if regime == "wide" else (0.02, 0.98)
    want, parts, c = {}, [], 2000
    for n in D_SIZES:
        parts.append(_cell_points(rng, n, c, h, lo, hi, yz_h=h))
        want[c] = n
        c += 37
    for na, nb in D_NEIGHBOURS:
        parts += [_cell_points(rng, na, c, h, lo, hi, yz_h=h), _cell_points(rng, nb, c + 1, h, lo, hi, yz_h=h)]
        want[c], want[c + 1] = na, nb
        c += 41
    xyz = np.concatenate([np.zeros((1, 3), np.float32), np.array([[anchor, 0, 0]], np.float32)] + parts)
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))], np.float32), C_TOL, want


# ---------------------------------------------------------------------------------------
# Family E: site offsets
# ---------------------------------------------------------------------------------------
E_FOD_TOLS = (4e-3, 3e-2)
E_FOD_SIZES = ((1, 0), (3, 0))
E_PATCH_TOL = 1e-3
E_VOXEL_CONFIGS = ((0.012, 0), ((0.004, 0.05, 0.012), 0), (10.0, 0), (0.05, 3))


@functools.lru_cache(maxsize=None)
def site_fod(offset: str):
    from geometry_edges_cases import OFFSETS, shifted

    return shifted(fod_cloud(), OFFSETS[offset])  # NaN / Inf records stay non-finite


@functools.lru_cache(maxsize=None)
def site_patch(offset: str):
    from geometry_edges_cases import OFFSETS, patch8000, shifted

    return shifted(patch8000(), OFFSETS[offset])


@functools.lru_cache(maxsize=None)
def site_fod_components(offset: str, tol: float):
    return components(site_fod(offset), tol)


@functools.lru_cache(maxsize=None)
def site_rgb_cloud(offset: str, n: int = 20000):
    """the coloured scan of tests/test_fod_filters.py moved by the offset in float32, with one NaN and
    one Inf record"""
    from geometry_edges_cases import OFFSETS
    from test_fod_filters import _rgb_cloud

    c = _rgb_cloud(n)
    off = np.asarray(OFFSETS[offset], np.float32)
    for d, name in enumerate("xyz"):
        c.points[name] = (c.points[name] + off[d]).astype(np.float32)
    c.points["x"][5] = np.nan
    c.points["y"][17] = np.inf
    return c


# ---------------------------------------------------------------------------------------
# Family F: the forest under contention
# ---------------------------------------------------------------------------------------
F_SPACING = F32(335544 / 2.0 ** 25)  # 0.01 cut to 19 significant bits: i * spacing is exact for i < 32


@functools.lru_cache(maxsize=None)
def lattice32():
    """(xyz, tol_joined, tol_apart): a 32^3 lattice whose neighbours are all exactly F_SPACING apart.
    At tol_apart = the spacing, float(tol^2) equals every neighbour's d2: nothing links; tol_joined has
    float(tol^2) one float step above it: one component."""
    a = (np.arange(32, dtype=np.float32) * F_SPACING).astype(np.float32)
    assert np.all(np.diff(a) == F_SPACING) and np.all(a.astype(np.float64) == np.arange(32) * float(F_SPACING))
    xyz = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    xyz = xyz[np.random.default_rng(61).permutation(len(xyz))]
    d2 = F32(F_SPACING * F_SPACING)
    tol_apart = float(F_SPACING)
    up = np.nextafter(d2, INF32)
    tol_joined = float(np.sqrt(np.float64(up)))
    while r2_of(tol_joined) < up:
        tol_joined = float(np.nextafter(tol_joined, np.inf))
    assert r2_of(tol_apart) == d2 and r2_of(tol_joined) == up
    return np.ascontiguousarray(xyz), tol_joined, tol_apart


@functools.lru_cache(maxsize=None)
def comb():
    """(xyz, tol, index range of the cut tooth's far part): a 2000-point spine along x with a 50-point
    tooth along y on every 20th point, spacing 0.009 at tolerance 0.01; one tooth is cut by a gap widened
    to the tolerance at float granularity (one step closer still links)."""
    tol, s = 0.01, F32(0.009)
    x = (s * np.arange(2000, dtype=np.float32)).astype(np.float32)
    spine = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    teeth = []
    cut = None
    for t, i in enumerate(range(0, 2000, 20)):
        y = (s * np.arange(1, 51, dtype=np.float32)).astype(np.float32)
        if t == 57:
            a = np.array([x[i], y[24], 0], np.float32)
            _, b = last_linked(a, [x[i], y[24] + F32(0.0099), 0], tol, 1)
            y[25:] = (b[1] + s * np.arange(25, dtype=np.float32)).astype(np.float32)
            cut = (2000 + 50 * t + 25, 2000 + 50 * t + 50)
        teeth.append(np.stack([np.full(50, x[i], np.float32), y, np.zeros(50, np.float32)], 1))
    xyz = np.concatenate([spine] + teeth).astype(np.float32)
    return np.ascontiguousarray(xyz), tol, cut
