"""The parameter cases of the align parity tests: mgicp_params fields away from their defaults.

Shared by tests/test_param_space_inputs.py (CPU: the oracle alone, and the premises of the table) and
tests/test_param_space_gpu.py (engine against oracle, setters on a live context, the target cache's
key).  Nothing here touches the engine.  Every cloud is cached, made once per process and read-only.

One table, CASES, maps a case's name to the engine's keyword arguments (mgicp_params fields) and the size
n of its scan_vs_cad(n, n) pair; oracle_kw() gives the oracle's names for the same values.

The recorded n is the first of N_CHOICES at which the case is admissible(): no outer iteration of the
CPU oracle has a delta within 1e-3 of 1, PCL's stop threshold.  That is a condition on the inputs: the
engine's sums are ordered differently from the oracle's default order, and a delta that prints as 1 may
fall on either side.  As the oracle ran here: every case is admissible at n = 2000, so every case records
2000 and none was dropped ("inner5" is not admissible at 5000: its third delta there is 1.0004).  The
oracle's iteration counts over the table are 0, 1, 2, 3, 4, 8, 9 and 16; "k32_gate5mm" ends on PCL's
exception in its second iteration (one correspondence left), after one iteration whose delta is 1.047.
(test_param_space_inputs.py keeps this true.)
"""
import functools

import numpy as np

N_CHOICES = (2000, 5000, 8000)
KNIFE_EDGE = 1e-3
SQRT_DBL_MAX = float(np.sqrt(np.finfo(np.float64).max))  # pcl::Registration's default corr_dist_threshold_
BFGS, GN = 0, 1  # MGICP_SOLVER_PCL_BFGS, MGICP_SOLVER_GN

# mgicp_params field -> ref.RefGICP keyword
ORACLE_NAME = {
    "max_iter": "max_iterations", "tf_eps": "transformation_epsilon", "rot_eps": "rotation_epsilon",
    "max_corr_dist": "max_corr_dist", "gicp_eps": "gicp_epsilon", "k": "k",
    "max_inner_iter": "max_inner_iterations", "fixed_iterations": "fixed_iterations", "solver": "solver",
}
DEFAULTS = dict(max_iter=100, tf_eps=4e-3, rot_eps=2e-3, max_corr_dist=0.04, gicp_eps=1e-3, k=20,
                max_inner_iter=20, fixed_iterations=0, solver=BFGS)

# name -> (engine keyword arguments, recorded n)
CASES = {
    "defaults": ({}, 2000),
    # the exact K instantiations (5, 20) and the rounded-up sentinel path (1, 7, 31, 32), both ends
    "k1": (dict(k=1), 2000),
    "k5": (dict(k=5), 2000),
    "k7": (dict(k=7), 2000),
    "k20": (dict(k=20), 2000),
    "k31": (dict(k=31), 2000),
    "k32": (dict(k=32), 2000),
    "eps1e-6": (dict(gicp_eps=1e-6), 2000),
    "eps1e-2": (dict(gicp_eps=1e-2), 2000),
    "eps1": (dict(gicp_eps=1.0), 2000),
    "inner1": (dict(max_inner_iter=1), 2000),
    "inner2": (dict(max_inner_iter=2), 2000),
    "inner5": (dict(max_inner_iter=5), 2000),
    "inner100": (dict(max_inner_iter=100), 2000),
    "tf0_iter8": (dict(tf_eps=0.0, max_iter=8), 2000),
    "tf1e-6_iter30": (dict(tf_eps=1e-6, max_iter=30), 2000),
    "tf1e-1": (dict(tf_eps=1e-1), 2000),
    "rot1e-6_iter30": (dict(rot_eps=1e-6, max_iter=30), 2000),
    "rot1": (dict(rot_eps=1.0), 2000),
    "iter1": (dict(max_iter=1), 2000),
    "iter2": (dict(max_iter=2), 2000),
    "fixed1_iter3": (dict(fixed_iterations=1, max_iter=3), 2000),
    "gate0": (dict(max_corr_dist=0.0), 2000),
    "gate5mm": (dict(max_corr_dist=0.005), 2000),
    "gate_pcl_default": (dict(max_corr_dist=SQRT_DBL_MAX), 2000),
    "k7_eps1e-2_inner5": (dict(k=7, gicp_eps=1e-2, max_inner_iter=5), 2000),
    "k32_gate5mm": (dict(k=32, max_corr_dist=0.005), 2000),
    "gn_inner1": (dict(solver=GN, max_inner_iter=1), 2000),
    "gn_inner20": (dict(solver=GN, max_inner_iter=20), 2000),
    "gn_k7_eps1e-2": (dict(solver=GN, k=7, gicp_eps=1e-2), 2000),
}
BFGS_CASES = tuple(c for c, (kw, _) in CASES.items() if kw.get("solver", BFGS) == BFGS)
GN_CASES = tuple(c for c in CASES if c not in BFGS_CASES)
# the rows that may not be dropped: every k, gicp_eps and max_inner_iter case
MUST_KEEP = tuple(c for c in CASES if c.startswith(("k", "eps", "inner")))
# every (k, gicp_eps) pair of the table: what the covariance kernels are run with
COV_PAIRS = tuple(sorted({(dict(DEFAULTS, **kw)["k"], dict(DEFAULTS, **kw)["gicp_eps"]) for kw, _ in CASES.values()}))
TINY_K = (1, 20, 32)


def engine_kw(case):
    return dict(CASES[case][0])


def oracle_kw(case):
    return {ORACLE_NAME[f]: v for f, v in CASES[case][0].items()}


def full(case):
    """every field of the case, the defaults filled in"""
    return dict(DEFAULTS, **CASES[case][0])


@functools.lru_cache(maxsize=None)
def clouds(n):
    """(scan, cad, T_true) of synth.scan_vs_cad(n, n), read-only"""
    from leica_point_cloud_processing_amd import synth

    scan, cad, Ttrue = synth.scan_vs_cad(n, n)
    for a in (scan, cad, Ttrue):
        a.setflags(write=False)
    return scan, cad, Ttrue


@functools.lru_cache(maxsize=None)
def tiny_pair(k):
    """(source, target) of exactly k points each: the n == k edge, where every point's k neighbours are the
    whole cloud.  The target fills a 2 cm cube; the source is the target turned by 0.05 rad about z through
    the cube's centre and shifted by 1 mm, so every point has its partner far inside the 4 cm gate."""
    g = np.random.Generator(np.random.PCG64(100 + k))
    tgt = np.array([1.0, 2.0, 0.5]) + g.uniform(0.0, 0.02, (k, 3))
    c, s = np.cos(0.05), np.sin(0.05)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    ctr = np.array([1.01, 2.01, 0.51])
    src = (tgt - ctr) @ R.T + ctr + np.array([1e-3, -5e-4, 5e-4])
    out = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_align(case, n=None):
    """(T, info with the trace) of the CPU oracle's align of `case` on clouds(n) (n None: the recorded n) in
    its default summation order.  Cached and shared: do not modify."""
    from oracle import ref

    n = CASES[case][1] if n is None else n
    scan, cad, _ = clouds(n)
    o = ref.RefGICP(**oracle_kw(case))
    o.set_source(scan)
    o.set_target(cad)
    T, info = o.align(want_trace=True)
    T.setflags(write=False)
    return T, info


def deltas(trace, tf_eps, rot_eps):
    """PCL's convergence figure of every outer iteration as mgicp_align applies it (mgicp_engine.hip, the
    ratio / c_delta loop; gicp.hpp computeTransformation): the largest of |prev - T| (a float difference)
    times 1 / rot_eps over the 3 x 3 block and times 1 / tf_eps over the last column and the last row,
    starting from prev = I.  The maximum is taken with `c_delta > delta` from delta = 0, so a NaN entry
    (tf_eps = 0 against an unchanged entry: inf * 0) never counts."""
    out = []
    prev = np.eye(4, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.full((4, 4), 1.0 / np.float64(tf_eps))
        ratio[:3, :3] = 1.0 / np.float64(rot_eps)
        for T in trace:
            T = np.asarray(T, np.float32)
            c = ratio * np.abs(prev - T).astype(np.float64)
            delta = 0.0
            for v in c.ravel():
                if v > delta:
                    delta = float(v)
            out.append(delta)
            prev = T
    return out


def stops_at(ds, max_iter, fixed_iterations):
    """the iteration count PCL's rule ends on, given the deltas of the iterations run (None: it goes on)"""
    for i, d in enumerate(ds, 1):
        if i >= max_iter if fixed_iterations else (i >= max_iter or d < 1):
            return i
    return None


def admissible(info, tf_eps, rot_eps):
    """no outer iteration of the oracle's align sits on PCL's stop threshold: |delta - 1| > 1e-3 for all"""
    return all(abs(d - 1.0) > KNIFE_EDGE for d in deltas(info["trace"], tf_eps, rot_eps))


def np_covariances(xyz, k, eps):
    """GICP::computeCovariances restated in NumPy: the k nearest points by float squared distance (ties: the
    lower index); their coordinates and the FLOAT products of their coordinates (PointXYZRGB's members are
    floats: `cov(0, 0) += pt.x * pt.x` rounds the product to a float, about 1e-7 of a squared coordinate
    against variances of 1e-4 and less, before the double accumulator takes it) summed in doubles in
    neighbour order; the sums over k, less the outer product of the mean; an fp64 SVD; the singular values
    replaced by (1, 1, eps).  Rows as ref.covariances: c00 c01 c02 c11 c12 c22."""
    p32 = np.ascontiguousarray(xyz, np.float32)
    out = np.zeros((len(p32), 6))
    for i in range(len(p32)):
        d = p32 - p32[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]  # float32, PCL's order
        nb = p32[np.lexsort((np.arange(len(p32)), d2))[:k]]
        mean = np.zeros(3)
        raw = np.zeros((3, 3))
        for pt in nb:  # sequential double sums of float terms
            mean += pt.astype(np.float64)
            raw += np.outer(pt, pt).astype(np.float64)  # float32 products, then widened
        mean /= k
        C = raw / k - np.outer(mean, mean)
        U = np.linalg.svd(C)[0]
        C = U @ np.diag([1.0, 1.0, eps]) @ U.T
        out[i] = C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]
    return out
