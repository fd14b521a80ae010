"""Cases and a NumPy reference of the pre-alignment transform's three calls (include/mi355x_gicp.h "the
pre-alignment transform"): mgicp_reject_ransac, mgicp_reject_one_to_one and mgicp_estimate_rigid_svd.

The reference restates the header's rules with other tools than the library's: float32 NumPy operations for
the distance of a correspondence (one rounding per operation, no FMA), a pure-Python MT19937, math.fsum for
the 15 sums and numpy.linalg.svd for the models.  It logs every decision it takes, so that
test_reject_inputs.py can show each of them to be FIRM: no rounding difference between this file and the
library can flip it.

Firm margin of an inlier test.  Under a float model T the library evaluates, per axis r,
    p_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3,  d_r = p_r - q_r,  d2 = (dx^2 + dz^2) + dy^2
in float.  With u = 2^-24 each operation is off by at most u times its result, so p_r is off by at most
4 u A_r with A_r = |T_r0 x| + |T_r1 y| + |T_r2 z| + |T_r3| (three products and three sums, first order), and
d_r by that plus u |d_r|.  This file's float32 evaluation is the same formula, so both agree bit for bit on
the SAME model; but the two models may differ by one float ulp per coefficient (2 u relative: the library's
Jacobi and fixed-tree sums against svd and fsum), which moves p_r by at most 2 u A_r more.  Hence, against
the fp64 value d2x of the formula at the reference's model,
    |d_r(float, either model) - d_r(exact)| <= e = 6 u A + u |d_r|  <= 8 u (A + |q|),   A = max_r A_r,
    |d2 - d2x| <= 2 sqrt(3 d2x) e + 3 e^2 + 4 u d2x  =: margin(d2x)
(the last term: three squarings and two sums, rounded up).  A decision is firm when |d2x - thr2| >
margin(d2x) + thr2 * rel, where rel covers a threshold that was itself derived from a median of such d2
(the refine's error_threshold): rel = margin(median) / median for that round, 0 for the caller's threshold.
A sample's distance test compares a float the two sides compute identically with sample_dist_thresh, which
differs between them only by fp64 rounding of a covariance whose entries carry a cancellation of about
|mean|^2 / spread^2 < 2^8 here: firm when off the threshold by more than 2^-40 of it.
"""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
F32 = np.float32
INT_MAX = 2 ** 31 - 1
DBL_EPS = float(np.finfo(np.float64).eps)


class MT19937:
    """the 32-bit Mersenne Twister of the standard (boost::mt19937, std::mt19937), seeded as they seed it"""

    def __init__(self, seed):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.idx = 624

    def __call__(self):
        if self.idx >= 624:
            mt = self.mt
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.idx = 0
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


# ---- the header's arithmetic ---------------------------------------------------------------------------
def d2_float(T, S, Q):
    """float32 squared distances of the pairs (S[i], Q[i]) under the float32 model T [3, 4]"""
    T = np.asarray(T, F32)
    S = np.asarray(S, F32).reshape(-1, 3)
    Q = np.asarray(Q, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = []
        for r in range(3):
            p = ((T[r, 0] * S[:, 0] + T[r, 1] * S[:, 1]) + T[r, 2] * S[:, 2]) + T[r, 3]
            d.append(p - Q[:, r])
        out = (d[0] * d[0] + d[2] * d[2]) + d[1] * d[1]
    assert out.dtype == F32
    return out


def d2_exact(T, S, Q):
    """(the formula in fp64 at the float model T, the magnitude A + |q| of the margin's derivation)"""
    T = np.asarray(T, F32).astype(np.float64)
    S = np.asarray(S, np.float64).reshape(-1, 3)
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    p = S @ T[:, :3].T + T[:, 3]
    A = (np.abs(S) @ np.abs(T[:, :3]).T + np.abs(T[:, 3]) + np.abs(Q)).max(axis=1)
    return ((p - Q) ** 2).sum(axis=1), A


def margin(d2x, A):
    e = 8 * U * A
    return 2 * np.sqrt(3 * d2x) * e + 3 * e * e + 4 * U * d2x


def inlier(d2, thr):
    """(double)d2 < thr * thr, strict"""
    return np.asarray(d2, F32).astype(np.float64) < thr * thr


def sums15(S, Q):
    """sum s, sum t, sum t_r s_c, correctly rounded"""
    S = np.asarray(S, F32).astype(np.float64).reshape(-1, 3)
    Q = np.asarray(Q, F32).astype(np.float64).reshape(-1, 3)
    out = [math.fsum(S[:, r]) for r in range(3)] + [math.fsum(Q[:, r]) for r in range(3)]
    out += [math.fsum(Q[:, r] * S[:, c]) for r in range(3) for c in range(3)]  # products of floats: exact
    return np.array(out, np.float64)


def sum_terms_abs(S, Q):
    """sum of |term| of each of the 15 sums (for the standard bound of a recursive sum)"""
    return sums15(np.abs(np.asarray(S, F32)), np.abs(np.asarray(Q, F32)))


def model_f64(sums, n):
    """the header's model of n pairs from their sums, before the rounding to float: [3, 4] float64"""
    sm, tm = sums[0:3] / n, sums[3:6] / n
    sigma = sums[6:15].reshape(3, 3) / n - np.outer(tm, sm)
    Um, _d, Vt = np.linalg.svd(sigma)
    s = np.ones(3)
    if np.linalg.det(Um) * np.linalg.det(Vt) < 0:
        s[2] = -1.0
    R = Um @ np.diag(s) @ Vt
    return np.hstack([R, (tm - R @ sm)[:, None]])


def model(sums, n):
    return model_f64(sums, n).astype(F32)


def sample_dist_thresh(P):
    """((sqrt(l0) + sqrt(l1) + sqrt(l2)) / 3)^2 over the covariance of the points P (normalised by their number)"""
    n = len(P)
    s = sums15(P, P)
    sm = s[0:3] / n
    cov = s[6:15].reshape(3, 3) / n - np.outer(sm, sm)
    sv = np.linalg.svd(cov, compute_uv=False)
    t = float(np.sqrt(sv).sum()) / 3.0
    return t * t


def pair_dist_float(a, b):
    d = np.asarray(b, F32) - np.asarray(a, F32)
    return F32((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


class Sampler:
    def __init__(self, m):
        self.gen = MT19937(12345)
        self.sh = list(range(m))
        self.log = []  # (float distance, threshold) of every pair test made

    def rnd(self):
        return self.gen() >> 1

    def sample(self, P, thresh):
        """a good sample of positions within 1000 draws, or None; P: the source point of every position"""
        m = len(self.sh)
        if m < 3:
            return None
        sh = self.sh
        for _ in range(1000):
            for i in range(3):
                j = i + self.rnd() % (m - i)
                sh[i], sh[j] = sh[j], sh[i]
            a, b, c = sh[0], sh[1], sh[2]
            good = True
            for x, y in ((a, b), (a, c), (b, c)):
                d = pair_dist_float(P[x], P[y])
                self.log.append((float(d), thresh))
                if not float(d) > thresh:
                    good = False
                    break
            if good:
                return [a, b, c]
        return None


def ransac(c):
    """mgicp_reject_ransac's rules on case c; the result carries the log of the decisions"""
    m = len(c.iq)
    S = c.src[c.iq] if m else np.zeros((0, 3), F32)
    Q = c.tgt[c.im] if m else np.zeros((0, 3), F32)
    thr = float(c.threshold)
    res = SimpleNamespace(keep=np.ones(m, bool), n_keep=m, T=np.eye(4, dtype=F32), n_iterations=0,
                          n_inliers_ransac=0, n_refine_rounds=0, final_error_threshold=thr, kept_all=True,
                          selections=[], samples=None, n_good_samples=0, outcome="m<3")
    if m < 3:
        return res
    sampler = Sampler(m)
    res.samples = sampler
    sthr = sample_dist_thresh(S)
    res.sample_thresh = sthr

    def select(T, t, rel):
        d2 = d2_float(T, S, Q)
        res.selections.append((np.array(T, F32), t * t, rel))
        keep = inlier(d2, t)
        return np.flatnonzero(keep), d2[keep].astype(np.float64)

    iterations, k, best, skipped = 0, 1.0, -INT_MAX, 0
    max_skip = c.max_iterations * 10
    best_model = None
    log_probability = math.log(1.0 - 0.99)
    res.outcome = "no model"
    while iterations < k and skipped < max_skip:
        smp = sampler.sample(S, sthr)
        if smp is None:
            break
        res.n_good_samples += 1
        T = model(sums15(S[smp], Q[smp]), 3)
        res.selections.append((T, thr * thr, 0.0))
        cnt = int(inlier(d2_float(T, S, Q), thr).sum())
        if cnt > best:
            best, best_model = cnt, T
            w = best * (1.0 / m)
            p = 1.0 - math.pow(w, 3.0)
            p = min(max(DBL_EPS, p), 1.0 - DBL_EPS)
            k = log_probability / math.log(p)
        iterations += 1
        if iterations > c.max_iterations:
            break
    res.n_iterations = iterations
    if best_model is None:
        return res
    inl, _d2 = select(best_model, thr, 0.0)
    res.n_inliers_ransac = len(inl)
    final, final_model, ok = inl, best_model, True
    if c.refine:
        err, rounds, changed, osc = thr, 0, False, False
        prev, new, sizes, cur, rel = inl, np.zeros(0, np.int64), [], best_model, 0.0
        while True:
            res.n_refine_rounds += 1
            if len(prev):
                cur = model(sums15(S[prev], Q[prev]), len(prev))
            sizes.append(len(prev))
            new, d2 = select(cur, err, rel)
            if len(new) == 0:
                rounds += 1
                if rounds >= 1000:
                    break
            else:
                med = float(np.sort(d2)[len(d2) >> 1])
                err = math.sqrt(min(thr * thr, 9.0 * (2.1981 * med)))
                if 9.0 * (2.1981 * med) < thr * thr:
                    dx, A = d2_exact(cur, S[new], Q[new])
                    rel = float((margin(dx, A) / np.maximum(dx, 1e-300)).max())
                else:
                    rel = 0.0
                changed = False
                prev, new = new, prev
                if len(new) != len(prev):
                    if len(sizes) >= 4 and sizes[-1] == sizes[-3] and sizes[-2] == sizes[-4]:
                        osc = True
                        break
                    changed = True
                else:
                    changed = not np.array_equal(prev, new)
            if not changed:
                break
            rounds += 1
            if not rounds < 1000:
                break
        res.final_error_threshold = err
        if len(new) == 0:
            ok, res.outcome = False, "refine failed: empty"
        elif osc:
            res.outcome = "oscillating"
        elif not changed:
            final, final_model, res.outcome = new, cur, "refined"
        else:
            ok, res.outcome = False, "refine failed: rounds"
    else:
        res.outcome = "no refine"
    res.n_inliers_final = len(final) if ok else 0
    if not ok or len(final) < 3:
        if ok:
            res.outcome = "fewer than 3"
        return res
    res.kept_all = False
    res.keep = np.zeros(m, bool)
    res.keep[final] = True
    res.n_keep = len(final)
    res.T = np.vstack([final_model, np.array([[0, 0, 0, 1]], F32)]).astype(F32)
    return res


def one_to_one(im, dist):
    """the positions of the survivors in ascending index_match: smallest distance, then lowest position"""
    best = {}
    for i, (t, d) in enumerate(zip(np.asarray(im).tolist(), np.asarray(dist, F32).tolist())):
        if t < 0:
            continue
        if t not in best or d < best[t][0]:
            best[t] = (d, i)
    return np.array([best[t][1] for t in sorted(best)], np.int32)


# ---- cases ---------------------------------------------------------------------------------------------
def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rigid_pair(seed, m, sigma, outliers=0.3, medium=0.0, extra=7):
    """source and target keypoint clouds and m correspondences: a rigid motion plus noise of `sigma` per
    axis (clipped at 3 sigma), a share `outliers` of gross mismatches (the target at least 6 from where the
    motion puts the source point), a share `medium` displaced by exactly 1.1 along a random direction"""
    rng = np.random.default_rng(seed)
    ns, nt = m + extra, m + extra + 3
    src = rng.uniform(-10, 10, (ns, 3)).astype(F32)
    R, t = _rotation(rng), rng.uniform(-3, 3, 3)
    iq = np.sort(rng.permutation(ns)[:m]).astype(np.int32)
    im = rng.permutation(nt)[:m].astype(np.int32)
    tgt = rng.uniform(-10, 10, (nt, 3)).astype(F32)
    kind = np.zeros(m, np.int8)
    n_out, n_med = int(outliers * m), int(medium * m)
    kind[rng.permutation(m)[:n_out + n_med]] = [1] * n_out + [2] * n_med
    for i in range(m):
        p = R @ src[iq[i]].astype(np.float64) + t
        if kind[i] == 0:
            tgt[im[i]] = (p + np.clip(rng.normal(0, sigma, 3), -3 * sigma, 3 * sigma)).astype(F32)
        elif kind[i] == 2:
            v = rng.normal(size=3)
            tgt[im[i]] = (p + 1.1 * v / np.linalg.norm(v)).astype(F32)
        else:
            while True:
                g = rng.uniform(-10, 10, 3)
                if np.linalg.norm(g - p) > 6.0:
                    break
            tgt[im[i]] = g.astype(F32)
    return src, tgt, iq, im, kind


def _case(src, tgt, iq, im, threshold=1.5, max_iterations=1000, refine=True, kind=None):
    return SimpleNamespace(src=np.ascontiguousarray(src, F32), tgt=np.ascontiguousarray(tgt, F32),
                           iq=np.asarray(iq, np.int32), im=np.asarray(im, np.int32), threshold=threshold,
                           max_iterations=max_iterations, refine=refine, kind=kind)


CLEAN_M = (3, 64, 65, 1000, 4099)
RANSAC_CASES = tuple(f"clean_{m}" for m in CLEAN_M) + (
    "shrink", "near_mismatches", "no_refine", "max_iterations_0", "max_iterations_1", "m_0", "m_1", "m_2",
    "identical_sources", "garbage")
_CASES = {}
_REFS = {}


def case(name):
    if name in _CASES:
        return _CASES[name]
    if name.startswith("clean_"):
        m = int(name[6:])
        src, tgt, iq, im, kind = _rigid_pair(100 + m, m, 0.01)
        c = _case(src, tgt, iq, im, kind=kind)
    elif name == "shrink":  # noise large enough that 9 * 2.1981 * median < 1.5^2: the refine tightens
        src, tgt, iq, im, kind = _rigid_pair(7, 500, 0.12)
        c = _case(src, tgt, iq, im, kind=kind)
    elif name == "near_mismatches":  # mismatches of 1.1 stay inliers: the set at 1.5 does not change, the refine
        # ends at its first round and the tightened threshold is never applied
        src, tgt, iq, im, kind = _rigid_pair(8, 600, 0.02, outliers=0.2, medium=0.1)
        c = _case(src, tgt, iq, im, kind=kind)
    elif name == "no_refine":
        src, tgt, iq, im, kind = _rigid_pair(9, 300, 0.01)
        c = _case(src, tgt, iq, im, refine=False, kind=kind)
    elif name.startswith("max_iterations_"):
        src, tgt, iq, im, kind = _rigid_pair(10, 300, 0.01, outliers=0.5)
        c = _case(src, tgt, iq, im, max_iterations=int(name[15:]), kind=kind)
    elif name in ("m_0", "m_1", "m_2"):
        src, tgt, iq, im, kind = _rigid_pair(11, 5, 0.01, outliers=0.0)
        m = int(name[2:])
        c = _case(src, tgt, iq[:m], im[:m], kind=kind[:m])
    elif name == "identical_sources":  # every pairwise sample distance is 0: no good sample
        src, tgt, iq, im, kind = _rigid_pair(12, 40, 0.01)
        src[:] = src[0]
        c = _case(src, tgt, iq, im, kind=kind)
    elif name == "garbage":  # no rigid relation at all: no model gathers 3 inliers
        rng = np.random.default_rng(13)
        src = rng.uniform(-10, 10, (6, 3)).astype(F32)
        tgt = rng.uniform(-40, 40, (6, 3)).astype(F32)
        c = _case(src, tgt, np.arange(6), rng.permutation(6), max_iterations=50)
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


def reference(name):
    """the reference run of a case, computed once and shared"""
    if name not in _REFS:
        _REFS[name] = ransac(case(name))
    return _REFS[name]


def non_firm(res, c):
    """(inlier tests, sample tests) of the reference run that are not firm"""
    bad_inlier = 0
    S, Q = c.src[c.iq], c.tgt[c.im]
    for T, thr2, rel in res.selections:
        dx, A = d2_exact(T, S, Q)
        bad_inlier += int((np.abs(dx - thr2) <= margin(dx, A) + thr2 * rel).sum())
    bad_sample = 0
    if res.samples is not None and res.samples.log:
        d, t = np.array(res.samples.log).T
        # a zero distance is never above a threshold that cannot be negative: firm whatever the threshold's bits
        bad_sample = int(((np.abs(d - t) <= t * 2.0 ** -40) & (d > 0)).sum())
    return bad_inlier, bad_sample


# ---- scoring cases: correspondences on the threshold and one float step either side -------------------
def score_case(m, n_models, seed=0):
    """clouds, correspondences, models [n_models, 4, 4] and a threshold.  The first model is the identity and
    the first correspondences' targets sit at distance exactly thr (d2 == thr^2: not an inlier), one float
    step inside and one outside; indices repeat; one model holds a NaN (it counts nothing)."""
    rng = np.random.default_rng(1000 + 7 * m + n_models + seed)
    thr = 1.5
    ns, nt = max(m // 2, 1) + 2, max(m // 3, 1) + 3
    src = rng.uniform(-4, 4, (ns, 3)).astype(F32)
    tgt = rng.uniform(-4, 4, (nt, 3)).astype(F32)
    iq = rng.integers(0, ns, m).astype(np.int32)  # repeats
    im = rng.integers(0, nt, m).astype(np.int32)
    # pairs on the threshold under the identity: source (0.5, 0, 0), every operation below exact or shown
    src[0] = (0.5, 0, 0)
    tgt[0] = (2, 0, 0)                                  # d = -1.5, d2 = 2.25 = thr^2: out
    tgt[1] = (np.nextafter(F32(2), F32(0)), 0, 0)       # d = -(1.5 - 2^-23), d^2 rounds to the float below 2.25: in
    tgt[2] = (2, 0, 2.0 ** -11)                         # 2.25 + 2^-22, the float above 2.25: out
    for j in range(min(m, 3)):
        iq[j], im[j] = 0, j
    models = np.zeros((n_models, 4, 4), F32)
    for b in range(n_models):
        M = np.eye(4)
        if b:
            M[:3, :3] = _rotation(rng)
            M[:3, 3] = rng.uniform(-1, 1, 3)
        models[b] = M.astype(F32)
    if n_models > 1:
        models[n_models // 2, 1, 2] = np.nan
    return src, tgt, iq, im, models, thr


def score_reference(src, tgt, iq, im, models, thr):
    S, Q = src[iq], tgt[im]
    return np.array([int(inlier(d2_float(M[:3], S, Q), thr).sum()) for M in models], np.int32)


# ---- one-to-one cases ----------------------------------------------------------------------------------
def o2o_case(name):
    """(index_match, distance, n_target)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("fan_"):  # that many correspondences onto target 5, others onto their own
        f = int(name[4:])
        im = np.concatenate([np.full(f, 5), np.arange(6, 16)]).astype(np.int32)
        d = rng.uniform(0.1, 9, len(im)).astype(F32)
        p = rng.permutation(len(im))
        return im[p], d[p], 20
    if name == "ties":  # equal distances, an exact zero and a -0.0 among them
        im = np.array([3, 3, 3, 1, 1, 0, 0, 7], np.int32)
        d = np.array([2.0, 1.0, 1.0, 4.0, 4.0, 0.0, -0.0, 5.0], F32)
        return im, d, 8
    if name == "negative_match":
        im = np.array([-1, 2, -1, 2, 0, -5], np.int32)
        d = np.array([0.5, 3.0, 0.1, 2.0, 1.0, 0.2], F32)
        return im, d, 3
    if name.startswith("m_"):
        m = int(name[2:])
        nt = max(m // 3, 1)
        return rng.integers(-1, nt, m).astype(np.int32), rng.integers(0, 50, m).astype(F32) / F32(8), nt
    raise KeyError(name)


O2O_CASES = ("fan_1", "fan_2", "fan_64", "fan_65", "ties", "negative_match", "m_0", "m_1", "m_64", "m_65", "m_4099")


# ---- SVD cases -----------------------------------------------------------------------------------------
def svd_case(name):
    """(src, tgt, iq, im)"""
    if name.startswith("noisy_"):
        m = int(name[6:])
        src, tgt, iq, im, _ = _rigid_pair(300 + m, m, 0.05, outliers=0.0)
        return src, tgt, iq, im
    if name == "integer_rigid":  # integer points, a 90-degree rotation and an integer shift: every sum exact
        rng = np.random.default_rng(21)
        src = rng.integers(-50, 50, (257, 3)).astype(F32)
        R = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64)
        tgt = (src.astype(np.float64) @ R.T + np.array([3, -7, 11])).astype(F32)
        idx = np.arange(257, dtype=np.int32)
        return src, tgt, idx, idx
    if name == "reflection":  # the target is the mirror image of the source: det(sigma) < 0
        rng = np.random.default_rng(22)
        src = rng.uniform(-5, 5, (200, 3)).astype(F32)
        tgt = src.copy()
        tgt[:, 2] = -tgt[:, 2]
        idx = np.arange(200, dtype=np.int32)
        return src, tgt, idx, idx
    raise KeyError(name)
