"""Feature sets and the reference of the correspondence tests (mgicp_match_features,
InitialAlignment::obtainCorrespondences).

Shared by tests/test_match_inputs.py (CPU: every case is what it claims to be, the reference agrees with an
independent fp64 brute force wherever fp64 can tell) and tests/test_match_gpu.py (engine vs reference).  Nothing
in this module touches the engine.  Every builder is cached: a case and its reference are made once per
process and must not be modified.

The reference is the arithmetic of include/mi355x_gicp.h itself: a float32 accumulator acc = acc + d * d over
the 33 bins in ascending order with d = S[:, b, None] - T[None, :, b].  NumPy's float32 operations are unfused
and correctly rounded, so every acc is the specified d2 bit for bit.  Target rows with a non-finite value are
left out, the argmin takes the first index among equal minima, a query is tied when acc == min more than once,
and the FLT_MAX rule and the max_distance rule are applied afterwards.  Nothing here has a tolerance.
"""
import functools

import numpy as np

import fpfh_cases as fc

BINS = 33
FLT_MAX = np.finfo(np.float32).max
DBL_MAX = float(np.finfo(np.float64).max)


class Ref:
    """match int32 [ns] (-1: none), distance float32 [ns] (NaN where match = -1), tied bool [ns] (a matched
    query whose minimum more than one valid target attains), best float32 [ns] (the minimum before the FLT_MAX
    and max_distance rules; +inf without a valid target, NaN for an invalid query), source_valid bool [ns],
    target_valid bool [nt], n_source_valid, n_target_valid, n_correspondences, n_tied."""


def d2_matrix(S, T):
    """the specified float32 d2 of every (row of S, row of T), finite rows only: [len(S), len(T)]"""
    S = np.ascontiguousarray(S[:, :BINS], np.float32)
    Tt = np.ascontiguousarray(T[:, :BINS].T, np.float32)
    acc = np.zeros((len(S), len(T)), np.float32)
    d = np.empty_like(acc)
    with np.errstate(over="ignore"):
        for b in range(BINS):
            np.subtract(S[:, b, None], Tt[b][None, :], out=d)
            np.multiply(d, d, out=d)
            np.add(acc, d, out=acc)
    return acc


def reference(S, T, max_distance=None, rows=64):
    S = np.asarray(S, np.float32)
    T = np.asarray(T, np.float32)
    ns, nt = len(S), len(T)
    r = Ref()
    r.source_valid = np.isfinite(S[:, :BINS]).all(1) if ns else np.zeros(0, bool)
    r.target_valid = np.isfinite(T[:, :BINS]).all(1) if nt else np.zeros(0, bool)
    tidx = np.flatnonzero(r.target_valid)
    Tv = T[tidx]
    r.best = np.full(ns, np.nan, np.float32)
    r.best[r.source_valid] = np.inf
    arg = np.full(ns, -1, np.int64)
    ties = np.zeros(ns, bool)
    sidx = np.flatnonzero(r.source_valid)
    if len(tidx):
        for c in range(0, len(sidx), rows):   # chunks over the source rows bound the memory
            sel = sidx[c:c + rows]
            acc = d2_matrix(S[sel], Tv)
            mn = acc.min(1)
            r.best[sel] = mn
            arg[sel] = tidx[acc.argmin(1)]    # the first index among equal minima
            ties[sel] = (acc == mn[:, None]).sum(1) > 1
    md = DBL_MAX if max_distance is None else float(max_distance)
    with np.errstate(over="ignore", invalid="ignore"):
        md2 = np.float64(md) * np.float64(md)
        ok = r.source_valid & (arg >= 0) & (r.best < FLT_MAX) & ~(r.best.astype(np.float64) > md2)
    r.match = np.where(ok, arg, -1).astype(np.int32)
    r.distance = np.where(ok, r.best, np.float32(np.nan)).astype(np.float32)
    r.tied = ties & ok
    r.n_source_valid = int(r.source_valid.sum())
    r.n_target_valid = int(r.target_valid.sum())
    r.n_correspondences = int(ok.sum())
    r.n_tied = int(r.tied.sum())
    return r


def d2_f64(S, T, rows=32):
    """an independent fp64 brute force: (best d2, its first index, the runner-up d2) per row of S over the rows of
    T (all finite); the runner-up is the second smallest value, equal to the best when that is attained twice"""
    S = np.asarray(S, np.float64)[:, :BINS]
    T = np.asarray(T, np.float64)[:, :BINS]
    best = np.zeros(len(S))
    arg = np.zeros(len(S), np.int64)
    second = np.full(len(S), np.inf)
    for c in range(0, len(S), rows):
        diff = S[c:c + rows, None, :] - T[None, :, :]
        D = np.einsum("ijk,ijk->ij", diff, diff)
        arg[c:c + rows] = D.argmin(1)
        if D.shape[1] > 1:
            part = np.partition(D, 1, axis=1)
            best[c:c + rows], second[c:c + rows] = part[:, 0], part[:, 1]
        else:
            best[c:c + rows] = D[:, 0]
    return best, arg, second


# ---------------------------------------------------------------------------------------
# the cases: name -> (source float32 [ns, 33], target float32 [nt, 33], max_distance | None)
# ---------------------------------------------------------------------------------------
SIZES_NS = (1, 63, 64, 65, 257)
SIZES_NT = (1, 63, 64, 65, 1023, 1025, 4099)
SIZES_CASES = tuple(f"sizes_{ns}_{nt}" for ns in SIZES_NS for nt in SIZES_NT)
MAXDIST_CASES = ("maxdist_zero", "maxdist_below", "maxdist_at", "maxdist_above", "maxdist_dblmax")
FPFH_CASES = ("kp_vs_3res", "3res_vs_kp", "kp_vs_kp", "nonfinite", "nonfinite_target_nan")
EDGE_CASES = ("all_target_nan", "nt0", "ns0", "ns1_nt1", "nt1")
CASES = FPFH_CASES + EDGE_CASES + SIZES_CASES + ("multi_block", "late_bins", "dups", "huge") + MAXDIST_CASES


@functools.lru_cache(maxsize=None)
def fpfh_rows(name):
    """the fp64 FPFH histograms of an fpfh_cases case, cast to float32: [keypoints, 33]"""
    h = np.ascontiguousarray(fc.case_histograms(name)[0].astype(np.float32))
    h.setflags(write=False)
    return h


def random_rows(rng, n):
    """random non-negative rows, each feature block of 11 bins scaled to sum 100 (an FPFH row's shape)"""
    x = rng.gamma(0.6, 1.0, (n, 3, 11)) + 1e-3
    x *= 100.0 / x.sum(2, keepdims=True)
    return x.reshape(n, BINS).astype(np.float32)


def with_target_nan(T, seed=41, share=0.05):
    """5 % of the rows NaN in one bin only: bin 0, 16 or 32 in turn"""
    rng = np.random.default_rng(seed)
    T = T.copy()
    rows = rng.choice(len(T), max(1, int(round(share * len(T)))), replace=False)
    T[rows, np.array([0, 16, 32])[np.arange(len(rows)) % 3]] = np.nan
    return T


def winner_case(nt, pos, seed=47):
    """one query and nt targets a long way from it, but for the one at `pos`: the unique winner"""
    rng = np.random.default_rng(seed)
    q = random_rows(rng, 1)
    T = random_rows(np.random.default_rng(seed + 1), nt)
    T[pos] = q[0]
    T[pos, 5] += np.float32(0.25)
    return q, T


LATE_NS, LATE_NT = 65, 1030


def late_bins():
    """65 queries and 1030 targets, all identical in bins 0 .. 31; a query's bin 32 is 50 + i, a target's
    116 + (nt - 1 - j): for every query the last target is the only nearest one, by bin 32 alone"""
    rng = np.random.default_rng(43)
    base = random_rows(rng, 1)[0]
    S = np.tile(base, (LATE_NS, 1))
    T = np.tile(base, (LATE_NT, 1))
    S[:, 32] = 50.0 + np.arange(LATE_NS)
    T[:, 32] = 116.0 + (LATE_NT - 1 - np.arange(LATE_NT))
    return S.astype(np.float32), T.astype(np.float32)


def dups():
    """every target row three times at scattered indices: each matched query is tied, the lowest index wins"""
    base = fpfh_rows("part_3res")[:400]
    rng = np.random.default_rng(44)
    T = np.tile(base, (3, 1))[rng.permutation(1200)]
    return fpfh_rows("part_kp")[:500], np.ascontiguousarray(T)


HUGE_EXPECT = (3, 3, -1, 3, 4, -1)
HUGE_TIED = (False, True, False, False, False, False)


def huge():
    """rows of magnitude 1e19 and 1e20: one term of 1e38 stays below FLT_MAX, four of them or one of 1e40 are
    +inf.  Targets: 0 = 1e19 e5; 1 = 1e19 (e0 + e1 + e2 + e3); 2 = 1e20 e7; 3 = e0; 4 = an ordinary row.
    Queries: 0 = zeros: target 3 at d2 = 1 (target 0 at 1e38, targets 1 and 2 at +inf);
    1 = 1e19 e6: targets 3 and 4 both at exactly float(1e19)^2 (their small terms are absorbed), target 0 at
        twice that, targets 1 and 2 at +inf: 3, tied;
    2 = -1e20 e0 and 5 = 1e20 e9: every d2 is +inf: none;
    3, 4 = copies of targets 3 and 4: d2 = 0."""
    rng = np.random.default_rng(45)
    T = np.zeros((5, BINS), np.float32)
    T[0, 5] = 1e19
    T[1, :4] = 1e19
    T[2, 7] = 1e20
    T[3, 0] = 1.0
    T[4] = random_rows(rng, 1)[0]
    S = np.zeros((6, BINS), np.float32)
    S[1, 6] = 1e19
    S[2, 0] = -1e20
    S[3:5] = T[3:]
    S[5, 9] = 1e20
    return S, T


def _maxdist(name):
    S, T = fpfh_rows("part_kp"), fpfh_rows("part_3res")
    # thresholds at the double square root of one query's d2 and either side of it
    root = float(np.sqrt(np.float64(case_reference("kp_vs_3res").distance[maxdist_query()])))
    md = {"maxdist_zero": 0.0, "maxdist_below": float(np.nextafter(root, 0.0)), "maxdist_at": root,
          "maxdist_above": float(np.nextafter(root, np.inf)), "maxdist_dblmax": DBL_MAX}[name]
    return S, T, md


def maxdist_query():
    """the query the max_distance thresholds are taken from: the one with the median positive d2"""
    ref = case_reference("kp_vs_3res")
    pos = np.flatnonzero((ref.match >= 0) & (ref.distance > 0))
    order = pos[np.argsort(ref.distance[pos], kind="stable")]
    return int(order[len(order) // 2])


@functools.lru_cache(maxsize=None)
def case(name):
    """(source, target, max_distance | None)"""
    empty = np.zeros((0, BINS), np.float32)
    if name == "kp_vs_3res":
        return fpfh_rows("part_kp"), fpfh_rows("part_3res"), None
    if name == "3res_vs_kp":
        return fpfh_rows("part_3res"), fpfh_rows("part_kp"), None
    if name == "kp_vs_kp":
        return fpfh_rows("part_kp"), fpfh_rows("part_kp"), None
    if name == "nonfinite":
        return fpfh_rows("nonfinite"), fpfh_rows("part_3res"), None
    if name == "nonfinite_target_nan":
        return fpfh_rows("nonfinite"), with_target_nan(fpfh_rows("part_3res")), None
    if name == "all_target_nan":
        T = fpfh_rows("part_3res")[:50].copy()
        T[np.arange(50), np.arange(50) % BINS] = np.nan
        return fpfh_rows("part_kp")[:100], T, None
    if name == "nt0":
        return fpfh_rows("part_kp")[:100], empty, None
    if name == "ns0":
        return empty, fpfh_rows("part_3res")[:100], None
    if name == "ns1_nt1":
        return fpfh_rows("part_kp")[5:6], fpfh_rows("part_3res")[7:8], None
    if name == "nt1":
        return fpfh_rows("part_kp")[:100], fpfh_rows("part_3res")[7:8], None
    if name in SIZES_CASES or name == "multi_block":
        ns, nt = (4099, 10007) if name == "multi_block" else (int(v) for v in name.split("_")[1:])
        rng = np.random.default_rng(1000 * ns + nt)
        return random_rows(rng, ns), random_rows(rng, nt), None
    if name == "late_bins":
        return late_bins() + (None,)
    if name == "dups":
        return dups() + (None,)
    if name == "huge":
        return huge() + (None,)
    if name in MAXDIST_CASES:
        return _maxdist(name)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    S, T, md = case(name)
    return reference(S, T, md)
