"""Clouds and references of the boundary-estimation tests (mgicp_boundary_points,
InitialAlignment::obtainBoundaryKeypoints).

Shared by tests/test_boundary_inputs.py (CPU: every cloud is what it claims to be, the float32 model of
the specified arithmetic stays within the bound of the fp64 truth) and tests/test_boundary_gpu.py (engine
vs reference).  Nothing in this module touches the engine.  Every builder is cached: a cloud and its
reference are made once per process and must not be modified.

The reference of a case is NumPy / SciPy alone.  Neighbour sets: cKDTree candidates (k + 8 or more, the
list certified complete), FLANN's float `d2_f32`, rows sorted by (d2, original index).  Per record
  * truth:  fp64 -- n / |n| of the float32 input normal, an orthonormal tangent basis of its own, arctan2,
            the largest cyclic gap of the sorted angles; sens = max over the members of
            |delta| / |delta projected on the tangent plane|;
  * model:  the float32 restatement of the arithmetic of include/mi355x_gicp.h.
BOUND_i = 2^-20 (1 + sens_i): an angle's error is the rounding of the two dot products (relative to
|delta|, so sens times 2^-24 each in the angle) plus atan2f's few ulps of an angle below pi (2^-22 per
ulp); a gap is the difference of two angles.  The prototype's model stayed below 3.9 * 2^-23 sens.
"""
import functools

import numpy as np

import normals_cases as nc
from cluster_edges_cases import d2_f32

THRESHOLD = 1.047        # InitialAlignment's setAngleThreshold
K_DEFAULT = 30           # its setKSearch
SENS_MAX = 2.0 ** 10     # records with a larger sens are not compared
LEFT_OUT_MAX = 0.005     # share of the records with a normal a case may leave out of a comparison
LOG_CAP = 60             # kBndCap: entries of a lane's candidate log (boundary_kernel)
FLT_MIN = np.float32(1.17549435e-38)
TWO_PI_F = np.float32(2.0) * np.float32(np.pi)


def bound(sens):
    return 2.0 ** -20 * (1.0 + sens)


# ---------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------
class Ref:
    """Per record of the cloud:
    nn int32 [n, k] (original indices in (d2, index) order, -1 padded), size int64 (members),
    decided bool (none of the four never-a-boundary-point rules applies),
    truth / model float64 / float32 [n] (max gap, NaN where not decided), sens float64,
    tie bool (float d2 of the k-th and (k+1)-th candidate are equal), n_le int64 (finite records with
    float d2 <= the k-th; 0 for non-finite records), n_finite int."""


def neighbour_rows(xyz, k):
    """(fin_idx, J [nf, k] positions in the finite points or -1, D2 [nf, k], tie [nf], n_le [nf])"""
    from scipy.spatial import cKDTree

    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin_idx = np.flatnonzero(np.isfinite(xyz).all(1))
    pts = xyz[fin_idx]
    nf = len(pts)
    J = np.full((nf, k), -1, np.int64)
    D2 = np.full((nf, k), np.inf, np.float32)
    tie = np.zeros(nf, bool)
    n_le = np.zeros(nf, np.int64)
    if nf == 0:
        return fin_idx, J, D2, tie, n_le
    p64 = pts.astype(np.float64)
    tree = cKDTree(p64)
    kk = min(nf, k + 8)
    todo = np.arange(nf)
    while len(todo):
        dist, cand = tree.query(p64[todo], k=kk)
        dist, cand = dist.reshape(len(todo), kk), cand.reshape(len(todo), kk)
        d2 = d2_f32(pts[todo][:, None, :], pts[cand])
        # rows sorted by (d2, index): by index, then stably by d2.  The index is the position in pts,
        # monotone in the original index
        o1 = np.argsort(cand, axis=1, kind="stable")
        cand_s, d2_s = np.take_along_axis(cand, o1, 1), np.take_along_axis(d2, o1, 1)
        o2 = np.argsort(d2_s, axis=1, kind="stable")
        cand_s, d2_s = np.take_along_axis(cand_s, o2, 1), np.take_along_axis(d2_s, o2, 1)
        kth = d2_s[:, min(k, kk) - 1].astype(np.float64)
        # complete: every record outside the list is farther (exactly) than the float k-th, with the
        # float expression's relative error of a few 2^-24 to spare
        complete = (kk == nf) | (dist[:, -1] ** 2 > kth * (1 + 1e-5))
        done = todo[complete]
        m = min(k, kk)
        J[done, :m] = cand_s[complete][:, :m]
        D2[done, :m] = d2_s[complete][:, :m]
        if kk > k:
            tie[done] = d2_s[complete][:, k - 1] == d2_s[complete][:, k]
        n_le[done] = (d2_s[complete] <= d2_s[complete][:, m - 1:m]).sum(1)
        todo = todo[~complete]
        if len(todo):
            assert kk < nf
            kk = min(nf, 2 * kk)
    return fin_idx, J, D2, tie, n_le


def _truth(pts, nrm, J, member):
    """fp64 max gap and sens per finite record (NaN / inf where there is no angle)"""
    p64 = pts.astype(np.float64)
    n = nrm.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.linalg.norm(n, axis=1)[:, None]
    # a tangent basis of the truth's own: e = n x (the axis of n's smallest component), f = n x e
    ax = np.eye(3)[np.argmin(np.abs(np.nan_to_num(n)), axis=1)]
    e = np.cross(n, ax)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = e / np.linalg.norm(e, axis=1)[:, None]
    f = np.cross(n, e)
    d = p64[np.maximum(J, 0)] - p64[:, None, :]
    use = member & (d != 0).any(2)
    with np.errstate(invalid="ignore", divide="ignore"):
        ang = np.arctan2((d * f[:, None, :]).sum(2), (d * e[:, None, :]).sum(2))
        tang = d - (d * n[:, None, :]).sum(2)[:, :, None] * n[:, None, :]
        s = np.linalg.norm(d, axis=2) / np.linalg.norm(tang, axis=2)
    sens = np.where(use, s, 0.0).max(1) if J.shape[1] else np.zeros(len(pts))
    ang = np.sort(np.where(use, ang, np.inf), axis=1)
    cp = use.sum(1)
    gap = np.full(len(pts), np.nan)
    for i in np.flatnonzero(cp > 0):
        a = ang[i, :cp[i]]
        gap[i] = max(np.diff(a).max(initial=0.0), 2 * np.pi - a[-1] + a[0])
    return gap, sens, cp


def _model(pts, nrm, J, member):
    """the float32 arithmetic of the header comment, one rounding per operation"""
    f32 = np.float32
    n = nrm.astype(f32)
    nf = len(pts)
    rows = np.arange(nf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        maxi = np.argmax(np.abs(np.nan_to_num(n, nan=0.0, posinf=3e38, neginf=3e38)), axis=1)  # first of the largest
        sndi = np.where(maxi == 0, 1, 0)
        ns, nm = n[rows, sndi], n[rows, maxi]
        inv = f32(1.0) / np.sqrt((ns * ns + nm * nm).astype(f32)).astype(f32)
        v = np.zeros((nf, 3), f32)
        v[rows, maxi] = -ns * inv
        v[rows, sndi] = nm * inv
        u = np.stack([n[:, 1] * v[:, 2] - n[:, 2] * v[:, 1], n[:, 2] * v[:, 0] - n[:, 0] * v[:, 2],
                      n[:, 0] * v[:, 1] - n[:, 1] * v[:, 0]], 1).astype(f32)
        d = (pts[np.maximum(J, 0)] - pts[:, None, :]).astype(f32)
        use = member & (d != 0).any(2)

        def dot(w):
            t = w[:, None, :] * d
            return ((t[:, :, 0] + t[:, :, 1]).astype(f32) + t[:, :, 2]).astype(f32)

        ang = np.arctan2(dot(v), dot(u)).astype(f32)
    ang = np.sort(np.where(use, ang, f32(np.inf)), axis=1)
    cp = use.sum(1)
    gap = np.full(nf, np.nan, f32)
    for i in np.flatnonzero(cp > 0):
        a = ang[i, :cp[i]]
        g = FLT_MIN
        for j in range(1, len(a)):
            dif = f32(a[j] - a[j - 1])
            if g < dif:
                g = dif
        dif = f32(f32(TWO_PI_F - a[-1]) + a[0])
        if g < dif:
            g = dif
        gap[i] = g
    return gap


def reference(xyz, normals, k):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32)[:, :3]
    n = len(xyz)
    fin_idx, J, _D2, tie, n_le = neighbour_rows(xyz, k)
    pts, nrm = xyz[fin_idx], normals[fin_idx]
    member = J >= 0
    r = Ref()
    r.n_finite = len(fin_idx)
    r.nn = np.full((n, k), -1, np.int32)
    r.nn[fin_idx] = np.where(member, fin_idx[np.maximum(J, 0)] if len(fin_idx) else -1, -1)
    r.size = np.zeros(n, np.int64)
    r.size[fin_idx] = member.sum(1)
    r.tie = np.zeros(n, bool)
    r.tie[fin_idx] = tie
    r.n_le = np.zeros(n, np.int64)
    r.n_le[fin_idx] = n_le
    r.truth = np.full(n, np.nan)
    r.model = np.full(n, np.nan, np.float32)
    r.sens = np.full(n, np.inf)
    r.decided = np.zeros(n, bool)
    if len(fin_idx):
        truth, sens, cp = _truth(pts, nrm, J, member)
        model = _model(pts, nrm, J, member)
        ok = np.isfinite(nrm).all(1) & (member.sum(1) >= 3) & (cp > 0)
        r.decided[fin_idx] = ok
        r.truth[fin_idx] = np.where(ok, truth, np.nan)
        r.model[fin_idx] = np.where(ok, model, np.float32(np.nan))
        r.sens[fin_idx] = np.where(ok, sens, np.inf)
    return r


def comparable(ref, thr=THRESHOLD):
    """(gap_ok, flag_ok): the decided records whose gap / whose flag is compared with the truth"""
    with np.errstate(invalid="ignore"):
        gap_ok = ref.decided & (ref.sens <= SENS_MAX)
        flag_ok = gap_ok & (np.abs(ref.truth - np.float64(np.float32(thr))) > bound(ref.sens))
    return gap_ok, flag_ok


# ---------------------------------------------------------------------------------------
# the cases: name -> (xyz float32 [n, 3], normals float32 [n, 3], k)
# ---------------------------------------------------------------------------------------
CASES = ("cube", "part", "part_small", "nonfinite", "huge_radius", "clump", "lattice", "outliers", "k7", "k32",
         "few", "dups", "one_angle", "pile") + nc.FAR_CASES
TIE_CASES = ("lattice", "pile", "lattice_rim")  # the cases built for float d2 ties across the k-th place


def truth_normals(xyz, radius):
    """the float32-rounded fp64 normals of normals_cases.reference (NaN where a record has none)"""
    return nc.reference(xyz, radius).normal.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _from_normals_case(name):
    xyz, radius = nc.case(name)
    return xyz, nc.case_reference(name).normal.astype(np.float32)


@functools.lru_cache(maxsize=None)
def lattice():
    """A 14 x 14 sheet at step 0.1 joined to a 14 x 5 wall, 266 points, exact normals: lattice distances
    tie in float d2 at the k-th place."""
    s = np.arange(14, dtype=np.float32) * np.float32(0.1)
    gx, gy = np.meshgrid(s, s, indexing="ij")
    sheet = np.stack([gx.ravel(), gy.ravel(), np.zeros(196, np.float32)], 1)
    wz = (np.arange(1, 6, dtype=np.float32) * np.float32(0.1))
    # the wall's columns stand half a step beside the sheet's, so no difference is parallel to a normal
    wx, wzz = np.meshgrid(s + np.float32(0.05), wz, indexing="ij")
    wall = np.stack([wx.ravel(), np.zeros(70, np.float32), wzz.ravel()], 1)
    xyz = np.concatenate([sheet, wall]).astype(np.float32)
    nrm = np.concatenate([np.tile([[0, 0, 1]], (196, 1)), np.tile([[0, 1, 0]], (70, 1))]).astype(np.float32)
    return xyz, nrm


@functools.lru_cache(maxsize=None)
def outliers():
    """3000 scan points plus 40 records tens of metres away: their 30-NN are far and, alone within the
    normal radius, they have NaN normals."""
    scan, res = nc._part_scan()
    rng = np.random.default_rng(11)
    far = rng.uniform(30.0, 60.0, (40, 3)) * rng.choice([-1.0, 1.0], (40, 3))
    xyz = np.concatenate([scan[:1500], far[:20], scan[1500:3000], far[20:]]).astype(np.float32)
    return xyz, truth_normals(xyz, 10.0 * res)


@functools.lru_cache(maxsize=None)
def few():
    """10 finite points (and two non-finite records) of a noisy sheet: every set has 10 members"""
    rng = np.random.default_rng(12)
    xy = rng.uniform(0, 1, (12, 2))
    xyz = np.concatenate([xy, 0.01 * rng.normal(size=(12, 1))], 1).astype(np.float32)
    xyz[3, 1] = np.nan
    xyz[8, 0] = np.inf
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (12, 1))
    return xyz, nrm


@functools.lru_cache(maxsize=None)
def dups():
    """every point of a 300-point noisy sheet three times (shuffled): members with delta = 0 are skipped"""
    rng = np.random.default_rng(13)
    xy = rng.uniform(0, 1, (300, 2))
    base = np.concatenate([xy, 0.3 * xy[:, :1] + 0.002 * rng.normal(size=(300, 1))], 1).astype(np.float32)
    order = rng.permutation(900)
    xyz = np.tile(base, (3, 1))[order]
    nrm = np.tile((np.array([-0.3, 0.0, 1.0]) / np.sqrt(1.09)).astype(np.float32), (900, 1))
    return np.ascontiguousarray(xyz), nrm


@functools.lru_cache(maxsize=None)
def one_angle():
    """a point three times and one distinct neighbour within k = 4 (one angle: the gap is 2 pi); the rest
    of the cloud is a far sheet.  Records 0-2 are the triple, record 3 the neighbour."""
    rng = np.random.default_rng(14)
    sheet = np.concatenate([rng.uniform(5, 6, (60, 2)), np.zeros((60, 1))], 1)
    xyz = np.concatenate([np.tile([[1.0, 1.0, 0.0]], (3, 1)), [[1.01, 1.002, 0.0]], sheet]).astype(np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(xyz), 1))
    return xyz, nrm


@functools.lru_cache(maxsize=None)
def pile():
    """a jittered 30 x 30 sheet with one of its points present 70 times: for the queries whose k-th
    neighbour is a copy, more than LOG_CAP records lie within the k-th distance, so the candidate log of
    boundary_kernel overflows and boundary_sorted_kernel finishes them."""
    rng = np.random.default_rng(15)
    gx, gy = np.meshgrid(np.arange(30) * 0.05, np.arange(30) * 0.05)
    sheet = np.stack([gx.ravel() + rng.uniform(-0.01, 0.01, 900), gy.ravel() + rng.uniform(-0.01, 0.01, 900),
                      1.0 + rng.normal(0, 1e-3, 900)], 1)
    xyz = np.concatenate([sheet[:400], np.tile(sheet[465:466], (69, 1)), sheet[400:]]).astype(np.float32)
    return xyz, truth_normals(xyz, 0.12)


@functools.lru_cache(maxsize=None)
def case(name):
    """(xyz, normals, k)"""
    if name in ("cube", "part", "part_small", "nonfinite", "huge_radius") + tuple(nc.FAR_PART_OFFSET):
        return _from_normals_case(name) + (K_DEFAULT,)
    # the far frames of normals_cases: a dense sheet whose grid slop is several cell edges (the stop test's
    # bound stays non-positive for the first rings, so ordinary queries may reach the ring cap and take the
    # hand-off), and the lattice whose d2 tie across the k-th place in a frame of 2^-11 steps
    if name in nc.FAR_SHEET_X0:
        return nc.far_sheet(name)[0], nc.far_sheet_normals(name), K_DEFAULT
    if name == "lattice_rim":
        return nc.lattice_rim()[0], nc.lattice_rim_normals(), K_DEFAULT
    if name == "clump":
        return _from_normals_case("clump") + (32,)
    if name == "k7":
        return _from_normals_case("part") + (7,)
    if name == "k32":
        return _from_normals_case("part") + (32,)
    if name == "one_angle":
        return one_angle() + (4,)
    return {"lattice": lattice, "outliers": outliers, "few": few, "dups": dups, "pile": pile}[name]() + (K_DEFAULT,)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    xyz, nrm, k = case(name)
    return reference(xyz, nrm, k)
