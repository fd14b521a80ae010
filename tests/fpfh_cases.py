"""Clouds and references of the FPFH tests (mgicp_fpfh_features, InitialAlignment::obtainFeatures).

Shared by tests/test_fpfh_inputs.py (CPU: every cloud is what it claims to be, the share of non-firm rows
stays under the cap, the float32 model of the specified arithmetic reproduces the truth bins of every firm
pair) and tests/test_fpfh_gpu.py (engine vs reference).  Nothing in this module touches the engine.  Every
builder is cached: a cloud and its reference are made once per process and must not be modified.

The reference of a case is NumPy / SciPy alone.  Neighbour sets: normals_cases.neighbour_pairs (cKDTree
candidates certified complete, FLANN's float `d2_f32`, strict).  Per ordered pair (i, j), j != i, of a
computed row:
  * truth:  computePairFeatures in fp64 from the float32 inputs as given (no renormalisation), the three
            brackets and their bins;
  * firm:   the truth bins survive the float arithmetic of include/mi355x_gicp.h.  With
            s = |dp x n1| / |dp|, a pair is NOT firm when a feature's bracket lies within
            TOL (1 + 1 / s) (f1, f2) or TOL (f3) of an interior bin edge k / 11, or when
            |acos|a1| - acos|a2|| < 4 TOL while the two branches give different bins or either branch is
            near an edge, or when s < TOL.  TOL = 2^-18: the float dots and the cross round at a few 2^-24
            relative to |dp|, normalising v amplifies that by 1 / s, atan2f / acosf add a few ulps of pi;
  * model:  the float32 restatement of the header's arithmetic (test_fpfh_inputs.py certifies TOL with it).
A row is firm when all its pairs are.
"""
import functools

import numpy as np

import boundary_cases as bc
import normals_cases as nc
from cluster_edges_cases import d2_f32

TOL = 2.0 ** -18
NONFIRM_CAP = 0.05   # largest share of non-firm rows among the computed rows of a case
MAX_SET = 65535      # the rows' uint16 limit
D_PI_F = np.float32(1.0) / (np.float32(2.0) * np.float32(np.pi))


def hist_bound(m):
    """|bin - fp64 evaluation| of a keypoint with m set members: four roundings per term, m terms per bin,
    11 m terms per feature sum, one division and one product; bins are on a scale of 100"""
    return 100.0 * (12.0 * m + 16.0) * 2.0 ** -24


class Ref:
    """n, n_finite; finite bool [n]; union bool [n] (records within the radius of some keypoint);
    size int64 [n] (m_i on the union, else 0); full_size int64 [n] (m_i of every finite record);
    counts int64 [n, 33] (truth, zero outside the union); nonfirm int64 [n] (non-firm pairs of the row);
    I, J (positions in the finite points of every ordered set pair, I == J included), d2 float32 per pair,
    fin_idx; pair_* arrays of the feature pairs (see pair_truth)."""


# ---------------------------------------------------------------------------------------
# pair features
# ---------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    with np.errstate(invalid="ignore"):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                         a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _bins(t):
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.floor(t), nan=0.0), 0, 10).astype(np.int64)


def _edge_dist(t):
    """distance of the bracket t / 11 from the nearest interior bin edge k / 11, k = 1 .. 10"""
    k = np.clip(np.rint(t), 1, 10)
    return np.abs(t - k) / 11.0


def _branch(n1, n2, dp, f3):
    """fp64 (t1, t2, t3, s) of one role assignment; rows with |dp x n1| = 0 give NaN and s = 0"""
    f4 = np.linalg.norm(dp, axis=1)
    v = _cross(dp, n1)
    vn = np.linalg.norm(v, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = vn / f4
        v = v / vn[:, None]
        w = _cross(n1, v)
        f2 = _dot(v, n2)
        f1 = np.arctan2(_dot(w, n2), _dot(n1, n2))
    t1 = 11.0 * ((f1 + np.pi) * (1.0 / (2.0 * np.pi)))
    t2 = 11.0 * ((f2 + 1.0) * 0.5)
    t3 = 11.0 * ((f3 + 1.0) * 0.5)
    return t1, t2, t3, s


def pair_truth(pi, ni, pj, nj):
    """fp64 features of the pairs (float32 inputs as given).  Returns (valid, bins [k, 3], firm):
    valid = the pair adds a count (f4 != 0, both normals finite, |v| != 0)."""
    pi, ni, pj, nj = (np.asarray(a, np.float32).astype(np.float64) for a in (pi, ni, pj, nj))
    k = len(pi)
    bins = np.zeros((k, 3), np.int64)
    if k == 0:
        return np.zeros(0, bool), bins, np.zeros(0, bool)
    dp = pj - pi
    f4 = np.linalg.norm(dp, axis=1)
    ok = (f4 != 0) & np.isfinite(ni).all(1) & np.isfinite(nj).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        a1 = _dot(ni, dp) / f4
        a2 = _dot(nj, dp) / f4
        swap = np.abs(a1) < np.abs(a2)          # acos|a1| > acos|a2|
        dacos = np.abs(np.arccos(np.minimum(np.abs(a1), 1.0)) - np.arccos(np.minimum(np.abs(a2), 1.0)))
    keep = _branch(ni, nj, dp, a1)
    swapped = _branch(nj, ni, -dp, -a2)

    def near(br):
        t1, t2, t3, s = br
        with np.errstate(invalid="ignore", divide="ignore"):
            lim = TOL * (1.0 + 1.0 / s)
            return ~((_edge_dist(t1) >= lim) & (_edge_dist(t2) >= lim) & (_edge_dist(t3) >= TOL) & (s >= TOL))

    def bins_of(br):
        return np.stack([_bins(br[0]), _bins(br[1]), _bins(br[2])], 1)

    bk, bs = bins_of(keep), bins_of(swapped)
    bins = np.where(swap[:, None], bs, bk)
    s = np.where(swap, swapped[3], keep[3])
    near_k, near_s = near(keep), near(swapped)
    firm = ~np.where(swap, near_s, near_k)
    tie = dacos < 4.0 * TOL
    firm &= ~(tie & ((bk != bs).any(1) | near_k | near_s))
    valid = ok & (s > 0)
    firm = np.where(ok, firm, True)  # a pair skipped on exact grounds (f4 = 0, a NaN normal) is firm
    bins[~valid] = 0
    return valid, bins, firm


def pair_model(pi, ni, pj, nj):
    """the float32 arithmetic of the header comment, one rounding per operation: (valid, bins [k, 3])"""
    f32 = np.float32
    pi, ni, pj, nj = (np.asarray(a, f32) for a in (pi, ni, pj, nj))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dp = (pj - pi).astype(f32)
        f4 = np.sqrt(_dot(dp * dp, np.ones_like(dp))).astype(f32)
        ok = (f4 != 0) & np.isfinite(ni).all(1) & np.isfinite(nj).all(1)
        a1 = (_dot(ni, dp) / f4).astype(f32)
        a2 = (_dot(nj, dp) / f4).astype(f32)
        swap = np.arccos(np.abs(a1)).astype(f32) > np.arccos(np.abs(a2)).astype(f32)
        n1 = np.where(swap[:, None], nj, ni)
        n2 = np.where(swap[:, None], ni, nj)
        dp = np.where(swap[:, None], -dp, dp)
        f3 = np.where(swap, -a2, a1).astype(f32)
        v = _cross(dp, n1).astype(f32)
        vn = np.sqrt(_dot(v * v, np.ones_like(v))).astype(f32)
        ok &= vn != 0
        v = (v / vn[:, None]).astype(f32)
        w = _cross(n1, v).astype(f32)
        f2 = _dot(v, n2).astype(f32)
        f1 = np.arctan2(_dot(w, n2).astype(f32), _dot(n1, n2).astype(f32)).astype(f32)
        ok &= ~(np.isnan(f1) | np.isnan(f2) | np.isnan(f3))
        t1 = 11.0 * ((f1.astype(np.float64) + np.pi) * np.float64(D_PI_F))
        t2 = 11.0 * ((f2.astype(np.float64) + 1.0) * 0.5)
        t3 = 11.0 * ((f3.astype(np.float64) + 1.0) * 0.5)
    bins = np.stack([_bins(t1), _bins(t2), _bins(t3)], 1)
    bins[~ok] = 0
    return ok, bins


# ---------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------
def reference(xyz, normals, keypoints, radius):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    normals = np.asarray(normals, np.float32).reshape(n, -1)[:, :3] if n else np.zeros((0, 3), np.float32)
    kp = np.arange(n) if keypoints is None else np.asarray(keypoints, np.int64)
    fin_idx, I, J = nc.neighbour_pairs(xyz, radius)
    pts, nrm = xyz[fin_idx], normals[fin_idx]
    nf = len(pts)
    r = Ref()
    r.n, r.n_finite, r.fin_idx, r.I, r.J = n, nf, fin_idx, I, J
    r.d2 = d2_f32(pts[I], pts[J]) if len(I) else np.zeros(0, np.float32)
    r.finite = np.zeros(n, bool)
    r.finite[fin_idx] = True
    pos = np.full(n, -1, np.int64)
    pos[fin_idx] = np.arange(nf)
    r.pos = pos
    size_f = np.bincount(I, minlength=nf).astype(np.int64) if nf else np.zeros(0, np.int64)
    r.full_size = np.zeros(n, np.int64)
    r.full_size[fin_idx] = size_f
    # the union of the keypoints' sets
    is_kp = np.zeros(nf, bool)
    kpf = pos[kp[r.finite[kp]]] if len(kp) else np.zeros(0, np.int64)
    is_kp[kpf] = True
    union_f = np.zeros(nf, bool)
    union_f[J[is_kp[I]]] = True
    r.union = np.zeros(n, bool)
    r.union[fin_idx] = union_f
    r.size = np.where(r.union, r.full_size, 0)
    # the feature pairs of the computed rows
    sel = union_f[I] & (I != J)
    pI, pJ = I[sel], J[sel]
    valid, bins, firm = pair_truth(pts[pI], nrm[pI], pts[pJ], nrm[pJ])
    r.pair_I, r.pair_J, r.pair_valid, r.pair_bins, r.pair_firm = pI, pJ, valid, bins, firm
    counts_f = np.zeros((nf, 33), np.int64)
    for f in range(3):
        np.add.at(counts_f, (pI[valid], 11 * f + bins[valid, f]), 1)
    r.counts = np.zeros((n, 33), np.int64)
    r.counts[fin_idx] = counts_f
    r.nonfirm = np.zeros(n, np.int64)
    r.nonfirm[fin_idx] = np.bincount(pI[~firm], minlength=nf) if nf else 0
    r.n_features = int(valid.sum())
    return r


def histograms(ref, keypoints, counts):
    """fp64 evaluation of the weighting formula per keypoint from bin counts [n, 33] (the truth's or the
    engine's), the reference's sets and sizes and the float d2: (hist [nk, 33], m [nk], firm [nk], lone
    [nk]); NaN rows for non-finite keypoints.  firm: every contributing row is firm."""
    n = ref.n
    kp = np.arange(n) if keypoints is None else np.asarray(keypoints, np.int64)
    counts = np.asarray(counts, np.float64)
    nf = ref.n_finite
    I, J, d2 = ref.I, ref.J, ref.d2.astype(np.float64)
    use = d2 != 0
    size_f = ref.full_size[ref.fin_idx].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(size_f > 1, 100.0 / (size_f - 1.0), 0.0)
    rows = counts[ref.fin_idx] * scale[:, None]          # the SPFH values of every finite record
    acc = np.zeros((nf, 33))
    np.add.at(acc, I[use], rows[J[use]] / d2[use][:, None])
    bad = np.zeros(nf, np.int64)
    np.add.at(bad, I[use], (ref.nonfirm[ref.fin_idx][J[use]] > 0).astype(np.int64))
    contributors = np.bincount(I[use], minlength=nf) if nf else np.zeros(0, np.int64)
    for f in range(3):
        s = acc[:, 11 * f:11 * f + 11].sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            acc[:, 11 * f:11 * f + 11] *= np.where(s != 0, 100.0 / s, 1.0)[:, None]
    nk = len(kp)
    hist = np.full((nk, 33), np.nan)
    m = np.zeros(nk, np.int64)
    firm = np.zeros(nk, bool)
    lone = np.zeros(nk, bool)
    fk = ref.finite[kp] if nk else np.zeros(0, bool)
    p = ref.pos[kp[fk]]
    hist[fk] = acc[p]
    m[fk] = ref.full_size[kp[fk]]
    firm[fk] = bad[p] == 0
    lone[fk] = contributors[p] == 0
    return hist, m, firm, lone


# ---------------------------------------------------------------------------------------
# the cases: name -> (xyz float32 [n, 3], normals float32 [n, 3], keypoints int32 | None, radius)
# ---------------------------------------------------------------------------------------
FAR_PART_CASES = {"far_part300_kp": ("far_part300", 1.4), "far_part300_3res": ("far_part300", 3.0),
                  "far_part4096_kp": ("far_part4096", 1.4), "far_part4096_3res": ("far_part4096", 3.0)}
FAR_CASES = tuple(nc.FAR_SHEET_X0) + tuple(FAR_PART_CASES) + ("lattice_rim",)
EDGE_VALUE_CASES = ("radius_zero", "n0", "n1", "n2", "n3")
CASES = ("part_kp", "part_3res", "part_all", "cube", "clump", "huge_radius", "nonfinite", "dups",
         "shuffled") + FAR_CASES + EDGE_VALUE_CASES
CLOUD_CASES = CASES[:-len(EDGE_VALUE_CASES)]     # the cases with neighbourhoods (the others are edge values)


@functools.lru_cache(maxsize=None)
def _part():
    """the part's scan, its truth normals (radius 10 resolutions) and the truth boundary keypoints"""
    scan, res = nc._part_scan()
    xyz, nrm, _k = bc.case("part")
    assert xyz is scan
    ref = bc.case_reference("part")
    with np.errstate(invalid="ignore"):
        kp = np.flatnonzero(ref.decided & (ref.truth > np.float64(np.float32(bc.THRESHOLD)))).astype(np.int32)
    return scan, nrm, kp, res


_tilted = nc.tilted


@functools.lru_cache(maxsize=None)
def cube():
    """the unit-test cube with its face normals at 5 resolutions, every record a keypoint: within a face
    a1 = a2 = 0, thousands of ties between the two role assignments that give the same bins"""
    xyz, _r = nc.cube()
    lo, hi = xyz.min(0), xyz.max(0)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    rel = (xyz - c) / half
    ax = np.argmax(np.abs(rel), axis=1)
    nrm = np.zeros_like(xyz)
    nrm[np.arange(len(xyz)), ax] = np.sign(rel[np.arange(len(xyz)), ax])
    return xyz, nrm.astype(np.float32), None, 5.0 * nc.resolution(xyz)


@functools.lru_cache(maxsize=None)
def clump():
    """normals_cases.clump at a radius of 6 mm: the sets of its 1500-point disc hold hundreds of records
    (above 255 and above a wave's 64 lanes), the sheet's records are alone"""
    xyz, _r = nc.clump()
    return xyz, _tilted(nc.case_reference("clump").normal, 23), None, 0.006


@functools.lru_cache(maxsize=None)
def huge_radius():
    """777 points (no multiple of 64) of a tilted sheet, a radius beyond the bounding box: one cell, every
    record in every set; every 7th record a keypoint.  A row has 776 pairs and a generic pair is non-firm
    about once in 10^4, so a row of generic pairs would rarely be firm: the sheet is nearly flat (noise a
    thousandth of its width) and the normals tilt by 0.02, which keeps the far pairs' features inside the
    middle bins; the near pairs still spread over the bins."""
    rng = np.random.default_rng(26)
    xy = rng.uniform(-0.5, 0.5, (777, 2))
    z = 2.0 + 0.2 * xy[:, 0] - 0.1 * xy[:, 1] + rng.normal(0, 0.001, 777)
    xyz = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    nrm = np.tile(np.array([-0.2, 0.1, 1.0]) / np.sqrt(1.05), (777, 1))
    return xyz, _tilted(nrm, 24), np.arange(0, 777, 7, dtype=np.int32), 10.0


@functools.lru_cache(maxsize=None)
def nonfinite():
    """NaN / Inf records, NaN normals (those of the non-finite records, of records with fewer than three
    neighbours and of 40 more), keypoints among all three kinds"""
    xyz, _r = nc.nonfinite()
    _scan, res = nc._part_scan()
    nrm = nc.case_reference("nonfinite").normal.astype(np.float32).copy()
    rng = np.random.default_rng(21)
    extra = rng.choice(len(xyz), 40, replace=False)
    nrm[extra[:20], 1] = np.nan
    nrm[extra[20:], :] = np.inf
    bad = np.flatnonzero(~np.isfinite(xyz).all(1))
    kp = np.concatenate([np.arange(0, len(xyz), 5), bad[:30], extra[:25]]).astype(np.int32)
    return xyz, nrm, kp, 3.0 * res


@functools.lru_cache(maxsize=None)
def dups():
    """boundary_cases.dups (every point of a 300-point sheet three times) with estimated normals: pairs
    with f4 = 0 and members with d2 = 0"""
    xyz, _n = bc.dups()
    return xyz, _tilted(bc.truth_normals(xyz, 0.15), 25), None, 0.1


@functools.lru_cache(maxsize=None)
def shuffled():
    """the part at 3 resolutions, its keypoints shuffled, a third of them twice"""
    scan, nrm, kp, res = _part()
    rng = np.random.default_rng(22)
    kp2 = np.concatenate([kp, kp[::3]])
    return scan, nrm, kp2[rng.permutation(len(kp2))].astype(np.int32), 3.0 * res


@functools.lru_cache(maxsize=None)
def _far_part(which):
    """_part()'s recipe in a site frame: the 3000 shifted records, their truth normals (radius 10
    resolutions), the truth boundary keypoints of that frame, the resolution"""
    xyz, nrm, _k = bc.case(which)
    ref = bc.case_reference(which)
    with np.errstate(invalid="ignore"):
        kp = np.flatnonzero(ref.decided & (ref.truth > np.float64(np.float32(bc.THRESHOLD)))).astype(np.int32)
    return xyz, nrm, kp, nc._far_part_base()[1]


def far_sheet(name):
    """normals_cases.far_sheet with its tilted plane normals at the normals' radius of 1.2 mm, every fifth
    record a keypoint: at |X0| = 4096.5 a record's cell box has 80-100 rows of cells -- fpfh_walk's outer
    loop takes a second turn of 64 rows -- where the control at X0 = 0 has at most 16"""
    xyz, radius = nc.far_sheet(name)
    return xyz, nc.far_sheet_normals(name), np.arange(0, len(xyz), 5, dtype=np.int32), radius


def lattice_rim():
    """normals_cases.lattice_rim with its tilted normals, every fifth record a keypoint: set sizes decided by
    pairs at d2 == r2 and one float step below"""
    xyz, radius = nc.lattice_rim()
    return xyz, nc.lattice_rim_normals(), np.arange(0, len(xyz), 5, dtype=np.int32), radius


@functools.lru_cache(maxsize=None)
def case(name):
    """(xyz, normals, keypoints | None, radius)"""
    if name in FAR_PART_CASES:
        which, factor = FAR_PART_CASES[name]
        xyz, nrm, kp, res = _far_part(which)
        return xyz, nrm, kp, factor * res
    if name in nc.FAR_SHEET_X0:
        return far_sheet(name)
    if name == "lattice_rim":
        return lattice_rim()
    if name in ("part_kp", "part_3res", "part_all"):
        scan, nrm, kp, res = _part()
        return scan, nrm, (None if name == "part_all" else kp), (1.4 if name == "part_kp" else 3.0) * res
    if name == "radius_zero":
        scan, nrm, kp, _res = _part()
        return scan[:500], nrm[:500], np.arange(0, 500, 3, dtype=np.int32), 0.0
    if name in ("n0", "n1", "n2", "n3"):
        k = int(name[1])
        xyz = np.array([[0, 0, 0], [0.01, 0.002, 0], [0, 0.01, 0.003]], np.float32)[:k]
        nrm = np.array([[0, 0, 1], [0.1, 0, 0.995], [0, -0.1, 0.995]], np.float32)[:k]
        return xyz, nrm, None, 0.05
    return {"cube": cube, "clump": clump, "huge_radius": huge_radius, "nonfinite": nonfinite, "dups": dups,
            "shuffled": shuffled}[name]()


@functools.lru_cache(maxsize=None)
def case_reference(name):
    xyz, nrm, kp, radius = case(name)
    return reference(xyz, nrm, kp, radius)


@functools.lru_cache(maxsize=None)
def case_histograms(name):
    """histograms() of the case from the truth counts"""
    _xyz, _nrm, kp, _radius = case(name)
    ref = case_reference(name)
    return histograms(ref, kp, ref.counts)


def nonfirm_share(ref):
    rows = int(ref.union.sum())
    return (float((ref.nonfirm[ref.union] > 0).sum()) / rows) if rows else 0.0
