"""Clouds and references of the radius-normal tests (mgicp_estimate_normals, Utils::getNormals).

Shared by tests/test_normals_inputs.py (CPU: every cloud is what it claims to be, the bounds the GPU
tests use hold for a NumPy model of the specified arithmetic) and tests/test_normals_gpu.py (engine vs
reference).  Nothing in this module touches the engine.  Every builder is cached: a cloud and its
reference are made once per process and must not be modified.

The reference of a case is NumPy / SciPy alone: cKDTree candidates, FLANN's float `dist2` expression for
the neighbour sets (exact counts), and per record
  * truth:  the fp64 normal / curvature of the set, from the CENTRED covariance and numpy.linalg.eigh;
  * model:  the arithmetic the engine is specified to use (fp64 raw moments of p_j - q_i, C = S/m - mu mu');
  * pcl:    PCL 1.8.1's arithmetic restated in float32 -- nine raw moments about the origin summed one
            after the other in FLANN's (d2, index) order, divided by m, centred in float -- whose
            eigenvector is then taken in fp64 (so its error is that of the sums alone: a lower bound).
`grid_of` (tests/cluster_edges_cases.py) restates the engine's cell index ONLY to certify that a cloud
reaches a regime of the kernel (a cell with more points than a block has lanes, a neighbourhood larger
than one staging chunk, a cell edge grown past the radius, a cell box widened by the slop of a far frame:
`box_facts`); it never produces an expected result.
"""
import functools
import os

import numpy as np

from cluster_edges_cases import cell_counts, d2_f32, grid_of, r2_of

BLOCK_LANES = 64     # kNrmThreads: queries one block holds
STAGE_POINTS = 512   # kNrmStage: points per staged chunk
GAP_MIN = 1e-2      # relative eigen-gap (l1 - l0) / l2 below which a normal is not compared
COS_MIN = 1e-3      # |cos| of truth normal and view direction below which the sign is not compared
DIR_BOUND = 2.0 ** -22   # angle <= DIR_BOUND / gap_rel
NORM_BOUND = 2.0 ** -22  # | |n| - 1 |
CURV_BOUND = 2.0 ** -21  # |curvature - truth|
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resolution(xyz):
    """Utils::computeCloudResolution's value to within float rounding: it only picks the cases' radii."""
    from scipy.spatial import cKDTree

    p = np.asarray(xyz, np.float64)
    d, _ = cKDTree(p).query(p, k=2)
    return float(d[:, 1].mean())


# ---------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------
class Ref:
    """Per record of the cloud (NaN / 0 where the record has no normal):
    count int64, has bool (finite and count >= 3), normal float64 [n, 3] (truth, sign as eigh gives it),
    curvature float64, gap_rel float64, model_angle / pcl_angle float64 (to the truth, sign ignored),
    model_curvature float64."""


def _angle(a, b):
    """angle between two directions, sign ignored, accurate near 0"""
    c = np.abs((a * b).sum(-1))
    s = np.linalg.norm(np.cross(a, b), axis=-1)
    return np.arctan2(s, c)


def _smallest(C):
    w, v = np.linalg.eigh(C)
    return w, v[:, :, 0]


def neighbour_pairs(xyz, radius):
    """(fin_idx, I, J): for the finite records pts = xyz[fin_idx], every ordered pair (I, J) of positions
    in pts with float d2 < float(radius^2) (I == J included), sorted by I then J."""
    from scipy.spatial import cKDTree

    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin_idx = np.flatnonzero(np.isfinite(xyz).all(1))
    pts = xyz[fin_idx]
    r2 = r2_of(radius)
    if len(pts) == 0 or not r2 > 0:
        return fin_idx, np.zeros(0, np.int64), np.zeros(0, np.int64)
    # a pair the float predicate accepts has an exact distance below sqrt(r2) (1 + 1e-6)
    reach = max(float(radius), float(np.sqrt(np.float64(r2))))
    p64 = pts.astype(np.float64)
    cand = cKDTree(p64).query_ball_point(p64, reach * (1 + 1e-5) + 1e-30)
    I = np.repeat(np.arange(len(pts)), [len(c) for c in cand])
    J = np.concatenate([np.asarray(c, np.int64) for c in cand]) if len(I) else np.zeros(0, np.int64)
    ok = d2_f32(pts[I], pts[J]) < r2
    I, J = I[ok], J[ok]
    order = np.lexsort((J, I))
    return fin_idx, I[order], J[order]


def reference(xyz, radius):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    fin_idx, I, J = neighbour_pairs(xyz, radius)
    pts = xyz[fin_idx]
    nf = len(pts)
    r = Ref()
    cnt_f = np.bincount(I, minlength=nf).astype(np.int64) if nf else np.zeros(0, np.int64)
    r.count = np.zeros(n, np.int64)
    r.count[fin_idx] = cnt_f
    r.has = r.count >= 3
    for name in ("curvature", "gap_rel", "model_angle", "pcl_angle", "model_curvature"):
        setattr(r, name, np.full(n, np.nan))
    r.normal = np.full((n, 3), np.nan)
    has_f = cnt_f >= 3
    if not has_f.any():
        return r
    keep = has_f[I]
    I, J = I[keep], J[keep]
    rows = np.flatnonzero(has_f)           # positions in pts that have a normal
    slot = np.full(nf, -1, np.int64)
    slot[rows] = np.arange(len(rows))
    S = slot[I]                            # pair -> row of the result arrays
    m = cnt_f[rows].astype(np.float64)
    p64 = pts.astype(np.float64)
    d = p64[J] - p64[I]                    # exact in fp64 for neighbouring floats
    k = len(rows)

    def seg(w):
        return np.bincount(S, weights=w, minlength=k)

    ij = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]

    def sym(c6):
        C = np.empty((k, 3, 3))
        for t, (a, b) in enumerate(ij):
            C[:, a, b] = C[:, b, a] = c6[t]
        return C

    mu = np.stack([seg(d[:, a]) for a in range(3)], 1) / m[:, None]
    # truth: centred second moments
    dc = d - mu[S]
    Ct = sym([seg(dc[:, a] * dc[:, b]) / m for a, b in ij])
    w, nt = _smallest(Ct)
    tr = w.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where(tr == 0, 0.0, np.abs(w[:, 0] / tr))
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    # model: the engine's specified arithmetic (raw moments of the differences, then S/m - mu mu')
    Cm = sym([seg(d[:, a] * d[:, b]) / m - mu[:, a] * mu[:, b] for a, b in ij])
    wm, nm = _smallest(Cm)
    trm = Cm[:, 0, 0] + Cm[:, 1, 1] + Cm[:, 2, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        curv_m = np.where(trm == 0, 0.0, np.abs(wm[:, 0] / trm))
    # pcl: float32 raw moments about the origin, one after the other in (d2, index) order
    d2 = d2_f32(pts[I], pts[J])
    order = np.lexsort((J, d2, I))
    q = pts[J[order]]
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    terms = np.stack([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z], 1).astype(np.float32)
    ends = np.cumsum(cnt_f[rows])
    starts = ends - cnt_f[rows]
    acc = np.empty((k, 9), np.float32)
    for t in range(k):  # np.cumsum adds sequentially in the array's type (np.sum would add pairwise)
        acc[t] = np.cumsum(terms[starts[t]:ends[t]], axis=0, dtype=np.float32)[-1]
    acc = (acc / cnt_f[rows].astype(np.float32)[:, None]).astype(np.float32)
    c6 = [(acc[:, t] - (acc[:, 6 + a] * acc[:, 6 + b]).astype(np.float32)).astype(np.float32)
          for t, (a, b) in enumerate(ij)]
    _, npcl = _smallest(sym([c.astype(np.float64) for c in c6]))
    at = fin_idx[rows]
    r.normal[at] = nt
    r.curvature[at] = curv
    r.gap_rel[at] = gap
    r.model_angle[at] = _angle(nm, nt)
    r.model_curvature[at] = curv_m
    r.pcl_angle[at] = _angle(npcl, nt)
    return r


def orientation(xyz, ref, viewpoint=(0.0, 0.0, 0.0)):
    """(sign, abs_cos) per record: the sign flipNormalTowardsViewpoint gives the truth normal (+1: kept,
    -1: flipped) and |cos| of the angle between the truth normal and the view direction."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        w = np.asarray(viewpoint, np.float32).astype(np.float64) - xyz.astype(np.float64)
        dot = (w * ref.normal).sum(1)
        cos = np.abs(dot) / np.linalg.norm(w, axis=1)
    return np.where(dot < 0, -1.0, 1.0), cos


def view_dot(xyz, normals, viewpoint=(0.0, 0.0, 0.0)):
    """(viewpoint - q) . n in fp64 over the float32 normals, added in the order x, y, z"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.asarray(viewpoint, np.float32).astype(np.float64) - xyz.astype(np.float64)
    nn = np.asarray(normals, np.float32).astype(np.float64)
    return (w[:, 0] * nn[:, 0] + w[:, 1] * nn[:, 1]) + w[:, 2] * nn[:, 2]


# ---------------------------------------------------------------------------------------
# the cases: name -> (xyz float32 [n, 3], radius)
# ---------------------------------------------------------------------------------------
FAR_SHEET_X0 = {"far_sheet": 4096.5, "far_sheet_neg": -4096.5, "far_sheet_origin": 0.0}
FAR_PART_OFFSET = {"far_part300": "site300", "far_part4096": "site4096"}  # keys of geometry_edges_cases.OFFSETS
FAR_CASES = tuple(FAR_SHEET_X0) + tuple(FAR_PART_OFFSET) + ("lattice_rim",)
DIRECTION_CASES = ("cube", "part", "part_small", "clump", "huge_radius", "tiny_radius", "nonfinite") + FAR_CASES
VIEWPOINT = (1.0, -2.0, 5.0)  # the non-default viewpoint of the `part` case


def _site_offset(name):
    from geometry_edges_cases import OFFSETS

    return OFFSETS[FAR_PART_OFFSET[name]]


def viewpoints():
    """name -> the non-default viewpoint of the case: VIEWPOINT, moved with the cloud in the far frames (the
    default one, the origin, is then kilometres away from the part)"""
    vp = {"part": VIEWPOINT, "far_sheet_origin": VIEWPOINT}  # the control's sheet passes through the origin
    for name in FAR_PART_OFFSET:
        vp[name] = tuple(float(v) for v in np.asarray(VIEWPOINT, np.float32) + np.asarray(_site_offset(name), np.float32))
    return vp


@functools.lru_cache(maxsize=None)
def cube():
    """The reference unit-test cube, 5000 points, radius 20 x resolution: dense neighbourhoods; the
    coordinates straddle the origin, so the default viewpoint lies inside the cloud."""
    from leica_point_cloud_processing_amd import synth

    src, _tgt, _T = synth.cube_fixture(os.path.join(ROOT, "tests", "golden", "cube.ply"))
    src = np.ascontiguousarray(src, np.float32)
    return src, 20.0 * resolution(src)


@functools.lru_cache(maxsize=None)
def _part_scan():
    from leica_point_cloud_processing_amd import synth

    scan, _cad, _T = synth.scan_vs_cad(6000, 6000)
    scan = np.ascontiguousarray(scan, np.float32)
    return scan, resolution(scan)


def part():
    scan, res = _part_scan()
    return scan, 10.0 * res


def part_small():
    """0.3 of the part's radius: 3-27 neighbours, some records with fewer than 3"""
    scan, res = _part_scan()
    return scan, 3.0 * res


@functools.lru_cache(maxsize=None)
def clump():
    """1500 points of a thin tilted disc 2 cm across in one spot, the rest (a jittered 40 x 40 sheet)
    metres away: one cell holds more points than a block has lanes and a neighbourhood is larger than
    one staging chunk."""
    rng = np.random.default_rng(5)
    nrm = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    u = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    v = np.cross(nrm, u)
    rad = 0.01 * np.sqrt(rng.random(1500))
    phi = rng.random(1500) * 2 * np.pi
    disc = (np.array([3.03, 1.02, 2.05]) + (rad * np.cos(phi))[:, None] * u + (rad * np.sin(phi))[:, None] * v +
            rng.normal(0, 2e-4, 1500)[:, None] * nrm)
    gx, gy = np.meshgrid(np.arange(40) * 0.05, np.arange(40) * 0.05)
    sheet = np.stack([gx.ravel() + rng.uniform(-0.01, 0.01, 1600), gy.ravel() + rng.uniform(-0.01, 0.01, 1600),
                      5.0 + rng.normal(0, 1e-3, 1600)], 1)
    xyz = np.concatenate([sheet[:800], disc, sheet[800:]]).astype(np.float32)
    return xyz, 0.12


@functools.lru_cache(maxsize=None)
def huge_radius():
    """777 points (no multiple of 64) of a noisy tilted sheet; the radius exceeds the bounding box: every
    point neighbours every point and the grid is one cell."""
    rng = np.random.default_rng(6)
    xy = rng.uniform(-0.5, 0.5, (777, 2))
    z = 2.0 + 0.2 * xy[:, 0] - 0.1 * xy[:, 1] + rng.normal(0, 0.01, 777)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32), 10.0


@functools.lru_cache(maxsize=None)
def tiny_radius():
    """A radius of 10 um against a bounding box 100 m long: the grid cannot have cells that small (2^20
    per axis), so its edge is grown past the radius.  600 points a sixth of a metre apart (all NaN) and
    six tilted planar patches of five points within the radius of each other (planar up to the float
    rounding of x, a hundredth of the patch's width)."""
    rng = np.random.default_rng(7)
    line = np.stack([np.linspace(0.0, 100.0, 600), rng.uniform(0, 5e-5, 600), rng.uniform(0, 5e-5, 600)], 1)
    patches = []
    for c in range(6):
        centre = np.array([0.11 + 0.13 * c, 2.5e-5, 2.5e-5])
        off = rng.uniform(-2.5e-6, 2.5e-6, (5, 2))
        patches.append(centre + np.stack([0.3 * off[:, 0] + 0.2 * off[:, 1], off[:, 0], off[:, 1]], 1))
    xyz = np.concatenate([line[:300]] + patches + [line[300:]]).astype(np.float32)
    return xyz, 1e-5


@functools.lru_cache(maxsize=None)
def nonfinite():
    """NaN and +-Inf records mixed into 3000 points of the part's scan (as
    test_covariance_path_nonfinite_records does)"""
    scan, res = _part_scan()
    bad = scan[:3000].copy()
    rng = np.random.default_rng(3)
    idx = rng.choice(len(bad), 50, replace=False)
    bad[idx[:20], 0] = np.nan
    bad[idx[20:35], 1] = np.inf
    bad[idx[35:45], 2] = -np.inf
    bad[idx[45:], :] = np.nan
    return bad, 14.0 * res


def tilted(nrm, seed, sigma=0.02):
    """unit normals tilted by a few hundredths of a radian each: on a flat patch estimated normals agree to
    the last bit, and two equal normals make a1 = a2 exactly -- a tie of the role assignment between
    branches with different f3 bins, which the firm flag rightly leaves out but a case must not consist of"""
    rng = np.random.default_rng(seed)
    t = nrm.astype(np.float64) + sigma * rng.normal(size=nrm.shape)
    with np.errstate(invalid="ignore"):
        return (t / np.linalg.norm(t, axis=1)[:, None]).astype(np.float32)


# ---- far frames (DESIGN.md "Site frames"): slop larger than the radius, site offsets, pairs at the rim
FAR_SHEET_RADIUS = 1.2e-3
FAR_SHEET_PLANE = (1.0, -0.3, 0.2)      # the sheet's normal, not normalised
LATTICE_RIM_STEP = 2.0 ** -11           # the float step of every coordinate of lattice_rim
LATTICE_RIM_OFF = (4096.5, -4100.25, 5000.75)
LATTICE_RIM_RADIUS = 5 * LATTICE_RIM_STEP


@functools.lru_cache(maxsize=None)
def far_sheet(name="far_sheet"):
    """6000 points of a noisy tilted sheet 3 cm x 3 cm, x = X0 + 0.3 y - 0.2 z + N(0, 5e-5), at a radius of
    1.2 mm.  At |X0| = 4096.5 the grid's slop (8 float steps of the largest coordinate, 3.9 mm) is three
    radii: a cell box is 9-10 cells wide where the same cloud at X0 = 0 (the control: the same draws) has
    boxes of at most 4 x 4 rows; x itself is cut to steps of 0.49 mm there.  -4096.5 is the mirrored side of
    every clamp and floor."""
    x0 = FAR_SHEET_X0[name]
    rng = np.random.default_rng(31)
    y = rng.uniform(0.0, 0.03, 6000)
    z = rng.uniform(0.0, 0.03, 6000)
    x = x0 + 0.3 * y - 0.2 * z + rng.normal(0.0, 5e-5, 6000)
    return np.ascontiguousarray(np.stack([x, y, z], 1), np.float32), FAR_SHEET_RADIUS


@functools.lru_cache(maxsize=None)
def far_sheet_normals(name="far_sheet"):
    """the sheet's plane normal, tilted by 0.02 rad per record: what the boundary and FPFH cases are given"""
    n = np.asarray(FAR_SHEET_PLANE) / np.linalg.norm(FAR_SHEET_PLANE)
    return tilted(np.tile(n, (6000, 1)), 33, sigma=0.02)


@functools.lru_cache(maxsize=None)
def _far_part_base():
    """the first 3000 records of the part's scan and their resolution (in the scan's own frame)"""
    scan, _res = _part_scan()
    base = np.ascontiguousarray(scan[:3000])
    return base, resolution(base)


@functools.lru_cache(maxsize=None)
def far_part(name):
    """3000 records of the part's scan moved by a site offset in float32, radius 10 resolutions: a
    metres-wide part whose coordinates have 2^-15 (site300) or 2^-11 m (site4096) steps"""
    from geometry_edges_cases import shifted

    base, res = _far_part_base()
    return shifted(base, _site_offset(name)), 10.0 * res


@functools.lru_cache(maxsize=None)
def lattice_rim_ij():
    """integer lattice coordinates of lattice_rim: 6000 draws in [0, 60) x [0, 60) x [0, 6), made unique,
    permuted"""
    rng = np.random.default_rng(41)
    ij = np.unique(rng.integers(0, [60, 60, 6], (6000, 3)), axis=0)
    return np.ascontiguousarray(ij[rng.permutation(len(ij))], np.int64)


@functools.lru_cache(maxsize=None)
def lattice_rim():
    """off + ij 2^-11 with every coordinate in [4096, 8192) in magnitude: each is a multiple of its float
    step, so every float d2 is an exact integer times 2^-22, and with radius = 5 steps float(radius^2) is
    exactly 25 of them.  Thousands of pairs sit at d2 == r2 (rejected: the test is strict) and one step below
    (24 = 16 + 4 + 4, accepted): the neighbour sets are decided by strictness alone, in a frame whose slop is
    two radii."""
    xyz64 = np.asarray(LATTICE_RIM_OFF) + lattice_rim_ij() * LATTICE_RIM_STEP
    xyz = xyz64.astype(np.float32)
    assert (xyz.astype(np.float64) == xyz64).all()
    return np.ascontiguousarray(xyz), LATTICE_RIM_RADIUS


@functools.lru_cache(maxsize=None)
def lattice_rim_normals():
    """(0.1, -0.2, 1) normalised, tilted by 0.05 rad per record"""
    n = np.array([0.1, -0.2, 1.0]) / np.sqrt(1.05)
    return tilted(np.tile(n, (len(lattice_rim_ij()), 1)), 43, sigma=0.05)


@functools.lru_cache(maxsize=None)
def degenerate():
    """Duplicated points and a collinear run, each out of reach of everything else, beside a small sheet.
    Returns (xyz, radius, rows): rows = the records whose neighbour set has no plane."""
    rng = np.random.default_rng(8)
    sheet = np.stack([rng.uniform(0, 1, 300), rng.uniform(0, 1, 300), 1.0 + rng.normal(0, 1e-3, 300)], 1)
    dup = np.tile(np.array([[5.0, 5.0, 5.0]]), (5, 1))
    dup2 = np.tile(np.array([[-3.0, 0.25, 7.0]]), (3, 1))
    run = np.array([8.0, -2.0, 1.0]) + np.arange(10)[:, None] * np.array([[0.01, 0.02, -0.005]])
    xyz = np.concatenate([sheet[:150], dup, run, dup2, sheet[150:]]).astype(np.float32)
    rows = np.arange(150, 150 + 5 + 10 + 3)
    return xyz, 0.06, rows


def edge_clouds():
    """name -> (xyz, radius) of the edge values: radius 0, a denormal float(radius^2), n = 0, 1, 2"""
    rng = np.random.default_rng(9)
    few = rng.uniform(0, 1, (40, 3)).astype(np.float32)
    dups = np.concatenate([few, few[:6], few[:3]]).astype(np.float32)  # three records thrice, three twice
    return {
        "radius_zero": (few, 0.0),
        "denormal_r2": (dups, 1e-20),          # float(1e-40) is denormal: only identical points are neighbours
        "n0": (np.zeros((0, 3), np.float32), 0.1),
        "n1": (few[:1], 0.1),
        "n2_near": (np.array([[0, 0, 0], [0.01, 0, 0]], np.float32), 0.1),
        "n2_far": (np.array([[0, 0, 0], [1, 0, 0]], np.float32), 0.1),
    }


def case(name):
    """(xyz, radius) of a direction case"""
    if name in FAR_SHEET_X0:
        return far_sheet(name)
    if name in FAR_PART_OFFSET:
        return far_part(name)
    if name == "lattice_rim":
        return lattice_rim()
    return {"cube": cube, "part": part, "part_small": part_small, "clump": clump, "huge_radius": huge_radius,
            "tiny_radius": tiny_radius, "nonfinite": nonfinite}[name]()


@functools.lru_cache(maxsize=None)
def case_reference(name):
    xyz, radius = case(name)
    return reference(xyz, radius)


def grid_facts(xyz, radius):
    """(h, largest cell population, per-axis dims) of the grid mgicp_estimate_normals builds: cell edge
    one radius, at most 2^20 cells per axis (restated by cluster_edges_cases.grid_of, whose edge is half
    its tolerance)."""
    g, _keys, counts = cell_counts(xyz, 2.0 * radius)
    return float(g.h), int(counts.max()), list(g.dims)


def box_facts(xyz, radius):
    """(rows, points, rx / h) of the cell box of every record taken as a single query (cell_box; a group of
    normals_tile_kernel has a box at least as large): rows of cells (y, z) and the points inside.  A float32
    restatement of rx = sqrtf(r2) * 1.0001f + slop, slop = 8 maxabs 2^-23 + 1e-6 h, over grid_of's cells.
    Like grid_of it only certifies that a cloud reaches a regime; it never produces an expected result."""
    f32 = np.float32
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    assert np.isfinite(xyz).all()
    g = grid_of(xyz, 2.0 * radius)
    slop = f32(f32(f32(8.0) * np.abs(xyz).max()) * f32(1.1920929e-7)) + f32(f32(1e-6) * f32(g.h))
    rx = f32(f32(np.sqrt(r2_of(radius))) * f32(1.0001)) + f32(slop)
    lo, hi = g.cells((xyz - rx).astype(f32)), g.cells((xyz + rx).astype(f32))
    rows = (hi[:, 1] - lo[:, 1] + 1) * (hi[:, 2] - lo[:, 2] + 1)
    nx, ny, nz = g.dims
    assert nx * ny * nz <= 1 << 24
    c = g.cells(xyz)
    cum = np.zeros((nx + 1, ny + 1, nz + 1), np.int64)  # cum[i, j, k]: points in cells below (i, j, k)
    np.add.at(cum, (c[:, 0] + 1, c[:, 1] + 1, c[:, 2] + 1), 1)
    cum = cum.cumsum(0).cumsum(1).cumsum(2)
    a, b = lo, hi + 1
    pts = np.zeros(len(xyz), np.int64)
    for sx, ix in ((1, b[:, 0]), (-1, a[:, 0])):
        for sy, iy in ((1, b[:, 1]), (-1, a[:, 1])):
            for sz, iz in ((1, b[:, 2]), (-1, a[:, 2])):
                pts += sx * sy * sz * cum[ix, iy, iz]
    return rows, pts, float(rx) / g.h
