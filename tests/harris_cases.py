"""Clouds and references of the Harris keypoint tests (mgicp_harris_keypoints,
InitialAlignment::obtainHarrisKeypoints).

Shared by tests/test_harris_inputs.py (CPU: every cloud is what it claims to be, the share of non-firm covar
entries stays under the cap, the float32 model of the response orders like fp64) and
tests/test_harris_gpu.py (engine vs reference).  Nothing in this module touches the engine.  Every builder
is cached: a cloud and its reference are made once per process and must not be modified.

The reference of a case is NumPy / SciPy alone.  Neighbour sets: normals_cases.neighbour_pairs (cKDTree
candidates certified complete, FLANN's float `d2_f32`, strict).  Per record i and covar entry k:
  * exact:  math.fsum of the float32 products of the counted members (the correctly rounded fp64 of their
            exact sum) divided by c_i in fp64 -- within 2 * 2^-53 sabs of the exact rational value,
            sabs = (sum of |product|) / c_i;
  * e:      (|N(i)| + 2) 2^-53 sabs: the engine's fp64 sum in any order and its division err by at most
            |N| 2^-53 sabs, the reference by the 2 above;
  * firm:   `exact` lies further than e from both float32 rounding midpoints around it, so the correctly
            rounded float is decided: float32(exact), bit for bit.  The other entries may differ by one ulp.
            An entry is firm as well when no fp64 operation can round (no_rounding): every product is a
            multiple of g = 2^(its lowest exponent - 23), and with (sum of |product|) < 2^53 g every partial
            sum, in any order or grouping, is such a multiple below 2^53 g, hence exact; and S / c is an fp64
            number.  The engine then holds the exact value too and float32(exact), ties to even, is its
            result.  Without this a set of two decides nothing: (p1 + p2) / 2 of two floats of one exponent
            IS a float32 midpoint half of the time, and at the reference's radius (1-8 neighbours) a sixth
            of all entries sit exactly on one.
The response model is the header's float32 expression, one rounding per operation (NumPy float32 arrays);
the keypoint rule is applied to whichever response array it is given.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import boundary_cases as bc
import normals_cases as nc

NONFIRM_CAP = 0.01          # largest share of non-firm covar entries among a case's entries
LANE_CAP = 512              # kHarLaneCap: candidates of a cell box a lane walks itself
THRESHOLD = np.float32(1e-6)  # detector.setThreshold(1e-6): PCL's threshold_ is a float
K004 = np.float32(0.04)


class Ref:
    """n, n_finite, fin_idx, finite bool [n]; I, J (positions in the finite points of every ordered set
    pair, I == J included); count int64 [n] (|N(i)|), c int64 [n]; exact float64 [n, 6], sabs float64 [n, 6],
    e float64 [n, 6], firm bool [n, 6], covar float32 [n, 6] (float32(exact)); response float32 [n] (the
    model on `covar`)."""


def response_model(covar):
    """the header's float32 expression, left to right, on covar float32 [n, 6]"""
    c = np.ascontiguousarray(covar, np.float32).reshape(-1, 6)
    xx, xy, xz, yy, yz, zz = (c[:, k] for k in range(6))
    two = np.float32(2.0)
    with np.errstate(invalid="ignore", over="ignore"):
        trace = (xx + yy) + zz
        det = (xx * yy) * zz
        det = det + ((two * xy) * xz) * yz
        det = det - (xz * xz) * yy
        det = det - (xy * xy) * zz
        det = det - (yz * yz) * xx
        r = (K004 + det) - (K004 * trace) * trace
    assert r.dtype == np.float32
    return np.where(trace != 0, r, np.float32(0.0)).astype(np.float32)


def response_fp64(covar):
    """the same expression in fp64 from the same float32 entries, and the sum of the magnitudes of its terms"""
    c = np.asarray(covar, np.float32).astype(np.float64).reshape(-1, 6)
    xx, xy, xz, yy, yz, zz = (c[:, k] for k in range(6))
    with np.errstate(invalid="ignore", over="ignore"):
        trace = xx + yy + zz
        terms = [xx * yy * zz, 2 * xy * xz * yz, xz * xz * yy, xy * xy * zz, yz * yz * xx]
        det = terms[0] + terms[1] - terms[2] - terms[3] - terms[4]
        r = 0.04 + det - 0.04 * trace * trace
        mag = 0.04 + sum(np.abs(t) for t in terms) + 0.04 * trace * trace
    return np.where(trace != 0, r, 0.0), mag


def keypoint_rule(ref, response, threshold, nonmax=True):
    """(keypoints int64 ascending, candidate bool [n], tied bool [n]) of the header's rule on `response`
    (float32 [n]) and the reference's sets.  tied: a keypoint whose response another member of its set
    equals."""
    n = ref.n
    resp = np.asarray(response, np.float32)
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        cand = ref.finite & np.isfinite(resp) & ~(resp < thr)
    if not nonmax:
        return np.arange(n, dtype=np.int64), cand, np.zeros(n, bool)
    ri, rj = resp[ref.fin_idx[ref.I]], resp[ref.fin_idx[ref.J]]
    with np.errstate(invalid="ignore"):
        lower = ri < rj
        same = (ri == rj) & (ref.I != ref.J)
    beaten = np.zeros(n, bool)
    beaten[ref.fin_idx[ref.I[lower]]] = True
    equalled = np.zeros(n, bool)
    equalled[ref.fin_idx[ref.I[same]]] = True
    key = cand & ~beaten
    return np.flatnonzero(key), cand, key & equalled


def reference(xyz, normals, radius):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    nrm = np.asarray(normals, np.float32).reshape(n, -1)[:, :3] if n else np.zeros((0, 3), np.float32)
    fin_idx, I, J = nc.neighbour_pairs(xyz, radius)
    nf = len(fin_idx)
    r = Ref()
    r.n, r.n_finite, r.fin_idx, r.I, r.J = n, nf, fin_idx, I, J
    r.finite = np.zeros(n, bool)
    r.finite[fin_idx] = True
    r.count = np.zeros(n, np.int64)
    r.c = np.zeros(n, np.int64)
    r.exact = np.zeros((n, 6))
    r.sabs = np.zeros((n, 6))
    r.no_rounding = np.zeros((n, 6), bool)
    if len(I):
        r.count[fin_idx] = np.bincount(I, minlength=nf)
        nj = nrm[fin_idx][J]
        counted = np.isfinite(nj[:, 0])
        cI, nj = I[counted], nj[counted]
        with np.errstate(invalid="ignore", over="ignore"):
            prod = np.stack([nj[:, 0] * nj[:, 0], nj[:, 0] * nj[:, 1], nj[:, 0] * nj[:, 2], nj[:, 1] * nj[:, 1],
                             nj[:, 1] * nj[:, 2], nj[:, 2] * nj[:, 2]], 1)
        assert prod.dtype == np.float32                    # each product rounded to float once
        prod = prod.astype(np.float64)
        cf = np.bincount(cI, minlength=nf)
        r.c[fin_idx] = cf
        start = np.concatenate([[0], np.cumsum(cf)])       # cI is sorted: a record's products are one run
        for p in np.flatnonzero(cf):
            rows = prod[start[p]:start[p + 1]]
            cnt = int(cf[p])
            for k in range(6):
                col = rows[:, k]
                if not np.isfinite(col).all():
                    with np.errstate(invalid="ignore"):
                        r.exact[fin_idx[p], k] = float(np.sum(col)) / cnt   # NaN or an infinity, whatever the order
                    continue
                s = math.fsum(col.tolist())
                sa = math.fsum(np.abs(col).tolist())
                q = s / cnt
                r.exact[fin_idx[p], k] = q
                r.sabs[fin_idx[p], k] = sa / cnt
                # every product is a multiple of g; sums below 2^53 g are exact in fp64 in any order
                nz = col[col != 0]
                if len(nz) == 0:
                    r.no_rounding[fin_idx[p], k] = True
                    continue
                g = 2.0 ** (int(np.frexp(np.abs(nz))[1].min()) - 24)
                r.no_rounding[fin_idx[p], k] = sa / g < 2.0 ** 53 and Fraction(q) * cnt == Fraction(s)
    with np.errstate(invalid="ignore", over="ignore"):
        r.covar = r.exact.astype(np.float32)
        r.e = (r.count[:, None] + 2.0) * 2.0 ** -53 * r.sabs
        lo = np.nextafter(r.covar, np.float32(-np.inf)).astype(np.float64)
        hi = np.nextafter(r.covar, np.float32(np.inf)).astype(np.float64)
        mid_lo, mid_hi = (r.covar.astype(np.float64) + lo) / 2, (r.covar.astype(np.float64) + hi) / 2
        far = (np.abs(r.exact - mid_lo) > r.e) & (np.abs(r.exact - mid_hi) > r.e)
    # an entry with c = 0 (exact zero) or a non-finite value is decided without arithmetic
    r.firm = far | r.no_rounding | ~np.isfinite(r.exact) | (r.c == 0)[:, None]
    r.response = response_model(r.covar)
    return r


def nonfirm_share(ref):
    rows = ref.finite
    total = int(rows.sum()) * 6
    return float((~ref.firm[rows]).sum()) / total if total else 0.0


# ---------------------------------------------------------------------------------------
# the cases: name -> (xyz float32 [n, 3], normals float32 [n, 3], radius, threshold float32, nonmax)
# ---------------------------------------------------------------------------------------
SCAN_CASES = {"cube_1p4": ("cube", 1.4), "cube_3": ("cube", 3.0), "cube_10": ("cube", 10.0),
              "part_1p4": ("part", 1.4), "part_3": ("part", 3.0), "part_10": ("part", 10.0)}
CLOUD_CASES = tuple(SCAN_CASES) + ("dups", "flat", "nonfinite", "lattice_rim", "far_part", "clump", "part_all")
EDGE_VALUE_CASES = ("radius_zero", "n0", "n1")
CASES = CLOUD_CASES + EDGE_VALUE_CASES
# the cases of the suppression test: each must hold suppressed candidates and keypoints (test_harris_inputs)
NMS_CASES = tuple(SCAN_CASES) + ("dups", "nonfinite", "lattice_rim", "far_part", "clump")


@functools.lru_cache(maxsize=None)
def _scan(which):
    """(xyz, fp64 NumPy normals at 20 resolutions rounded to float32, resolution) of the cube fixture
    (5000 points) or the synthetic part (6000 points)"""
    if which == "cube":
        xyz, radius = nc.cube()
        return xyz, nc.case_reference("cube").normal.astype(np.float32), radius / 20.0
    xyz, res = nc._part_scan()
    return xyz, bc.truth_normals(xyz, 20.0 * res), res


@functools.lru_cache(maxsize=None)
def dups():
    """boundary_cases.dups (every point of a 300-point sheet three times, shuffled) with estimated, tilted
    normals: the three copies of a point have one set, so one covar and one response -- a copy that is a
    keypoint brings its two twins along"""
    xyz, _n = bc.dups()
    return xyz, nc.tilted(bc.truth_normals(xyz, 0.15), 25, sigma=0.2), 0.1, THRESHOLD, 1


@functools.lru_cache(maxsize=None)
def flat():
    """700 points of a sheet (two of them non-finite records), one normal for all: every sum is c times
    one product, exact in fp64, so covar -- and the response -- has the same bits everywhere and, with a
    threshold of -1, every finite record is a keypoint tied with its whole set"""
    rng = np.random.default_rng(51)
    xyz = np.concatenate([rng.uniform(0, 1, (700, 2)), 0.01 * rng.normal(size=(700, 1))], 1).astype(np.float32)
    xyz[17, 2] = np.nan
    xyz[401, 0] = -np.inf
    nrm = np.tile((np.array([0.1, -0.2, 1.0]) / np.sqrt(1.05)).astype(np.float32), (700, 1))
    return xyz, nrm, 0.08, np.float32(-1.0), 1


@functools.lru_cache(maxsize=None)
def nonfinite():
    """normals_cases.nonfinite (NaN / Inf records in 3000 scan points) and its estimated normals at 3
    resolutions, with 20 more normals all NaN (not counted), 20 with a finite x and a NaN y (counted: the
    NaN goes through the sums of every set they are in: NaN response, no keypoint, nothing suppressed), 10
    with an infinite z; and three records far from the rest whose normals are all NaN: c = 0, covar and
    response 0"""
    xyz, _r = nc.nonfinite()
    _scan_, res = nc._part_scan()
    nrm = nc.case_reference("nonfinite").normal.astype(np.float32).copy()
    rng = np.random.default_rng(52)
    fin = np.flatnonzero(np.isfinite(xyz).all(1) & np.isfinite(nrm).all(1))
    extra = rng.choice(fin, 50, replace=False)
    nrm[extra[:20], :] = np.nan
    nrm[extra[20:40], 1] = np.nan
    nrm[extra[40:], 2] = np.inf
    lone = (np.array([50.0, -40.0, 30.0]) + 0.2 * res * rng.normal(size=(3, 3))).astype(np.float32)
    xyz = np.concatenate([xyz[:1000], lone, xyz[1000:]])
    nrm = np.concatenate([nrm[:1000], np.full((3, 3), np.nan, np.float32), nrm[1000:]])
    return np.ascontiguousarray(xyz), np.ascontiguousarray(nrm), 3.0 * res, THRESHOLD, 1


NONFINITE_LONE = (1000, 1001, 1002)


@functools.lru_cache(maxsize=None)
def lattice_rim():
    """normals_cases.lattice_rim with its tilted normals: set sizes decided by pairs at d2 == r2 and one
    float step below, in a frame whose slop is two radii"""
    xyz, radius = nc.lattice_rim()
    return xyz, nc.tilted(nc.lattice_rim_normals(), 53, sigma=0.2), radius, THRESHOLD, 1


@functools.lru_cache(maxsize=None)
def far_part():
    """3000 records of the part in the site4096 frame (coordinate steps of 2^-11 m) with their NumPy normals,
    at 3 resolutions"""
    xyz, nrm, _k = bc.case("far_part4096")
    return xyz, nrm, 3.0 * nc._far_part_base()[1], THRESHOLD, 1


@functools.lru_cache(maxsize=None)
def clump():
    """normals_cases.clump at a radius of 8 mm, normals tilted by 0.2 rad: the sets of the disc's 1500
    records hold up to a thousand records and their cell boxes more than kHarLaneCap candidates -- both
    sweeps hand them to the wave kernels -- while the sheet's records stay with the lanes"""
    xyz, _r = nc.clump()
    return xyz, nc.tilted(nc.case_reference("clump").normal, 54, sigma=0.2), 0.008, THRESHOLD, 1


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SCAN_CASES:
        which, factor = SCAN_CASES[name]
        xyz, nrm, res = _scan(which)
        return xyz, nrm, factor * res, THRESHOLD, 1
    if name == "part_all":                      # nonmax = 0: PCL's branch lists every record
        xyz, nrm, res = _scan("part")
        return xyz, nrm, 1.4 * res, THRESHOLD, 0
    if name == "radius_zero":
        xyz, nrm, _res = _scan("part")
        return xyz[:500], nrm[:500], 0.0, THRESHOLD, 1
    if name in ("n0", "n1"):
        k = int(name[1])
        return (np.array([[0.5, -0.25, 2.0]], np.float32)[:k], np.array([[0.6, 0.0, 0.8]], np.float32)[:k], 0.05,
                np.float32(-1.0), 1)
    return {"dups": dups, "flat": flat, "nonfinite": nonfinite, "lattice_rim": lattice_rim, "far_part": far_part,
            "clump": clump}[name]()


@functools.lru_cache(maxsize=None)
def case_reference(name):
    xyz, nrm, radius, _thr, _nonmax = case(name)
    return reference(xyz, nrm, radius)
