"""GICPEngine: the MI355X GICP behind pcl::GeneralizedIterativeClosestPoint's API surface.

Mirrors the subset of pcl::GeneralizedIterativeClosestPoint<PointXYZRGB,PointXYZRGB> that
GICPAlignment uses (/root/reference/src/GICPAlignment.cpp:48-54, 89-105, 116-123):
setMaximumIterations, setMaxCorrespondenceDistance, setTransformationEpsilon,
setRANSACOutlierRejectionThreshold (stored, unused by GICP), setInputSource, setInputTarget,
align, hasConverged, getFinalTransformation, getFitnessScore, getMaximumIterations.
All compute goes through libmgicp.so (include/mi355x_gicp.h); nothing runs on the CPU.
"""
from __future__ import annotations

import atexit
import ctypes

import numpy as np

from . import _lib
from .cloud import PointCloudRGB

DBL_MAX = float(np.finfo(np.float64).max)
_LIVE: set = set()
_SHUTTING_DOWN = [False]


@atexit.register
def _mark_shutdown():
    _SHUTTING_DOWN[0] = True


def _cm(T) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).T).reshape(16)


def _from_cm(buf) -> np.ndarray:
    return np.asarray(buf, dtype=np.float32).reshape(4, 4).T.copy()


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class GICPEngine:
    # mgicp_debug_option forms applied to every new engine before its own `options` (the GPU test suite
    # sets {"target_cache": 0} so engines of different tests never adopt each other's targets)
    DEFAULT_OPTIONS: dict = {}

    def __init__(self, device: int = -1, options: dict | None = None, **params):
        """params: mgicp_params fields; options: mgicp_debug_option forms (tests / diagnostics only)"""
        self._lib = _lib.load()
        self.params = _lib.default_params()
        self.params.device = device
        for k, v in params.items():
            setattr(self.params, k, v)
        h = ctypes.c_void_p()
        rc = self._lib.mgicp_create(ctypes.byref(h), ctypes.byref(self.params))
        if rc != 0:
            raise _lib.MgicpError(rc, "mgicp_create failed (no HIP device or invalid parameters)")
        self._h = h
        self._pushed = type(self.params).from_buffer_copy(self.params)  # what the context holds
        _LIVE.add(id(self))
        self.ransac_outlier_threshold = 0.05
        self._input = None
        self._converged = False
        self._final = np.eye(4, dtype=np.float32)
        self.last_result = None
        self.last_dominant_ms = None  # dominant_normals: ms from its first launch to the result on the host
        for k, v in {**GICPEngine.DEFAULT_OPTIONS, **(options or {})}.items():
            self.debug_option(k, v)

    def cache_stats(self) -> dict:
        """The process-wide target cache (mgicp_debug_cache_stats)."""
        out = (ctypes.c_longlong * 5)()
        self._check(self._lib.mgicp_debug_cache_stats(self._h, out), "cache_stats")
        return {"adopted": int(out[0]), "hits": int(out[1]), "donations": int(out[2]), "cached": int(out[3]),
                "source_spec": ("none", "pending", "kept", "discarded")[int(out[4])]}

    @staticmethod
    def release_cache():
        """Free the process-wide target cache (mgicp_release_cache)."""
        _lib.load().mgicp_release_cache()

    def debug_option(self, name: str, value):
        """mgicp_debug_option: a test / diagnostic form of the engine on this context only"""
        self._check(self._lib.mgicp_debug_option(self._h, name.encode(), float(value)), f"debug option {name}")

    def close(self):
        """Release the device context (deterministically, before interpreter shutdown)."""
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            _LIVE.discard(id(self))
            self._lib.mgicp_destroy(h)

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be torn down: leave the context
        # to the process exit instead of racing the runtime's own destructors
        if not _SHUTTING_DOWN[0]:
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- helpers -------------------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc < 0:
            raise _lib.MgicpError(rc, f"{what}: {self._lib.mgicp_last_error(self._h).decode()}")
        return rc

    def _push_params(self):
        rc = self._lib.mgicp_set_params(self._h, ctypes.byref(self.params))
        if rc < 0:  # refused: the context keeps its parameters, and so does this object
            ctypes.memmove(ctypes.byref(self.params), ctypes.byref(self._pushed), ctypes.sizeof(self.params))
        self._check(rc, "mgicp_set_params")
        self._pushed = type(self.params).from_buffer_copy(self.params)

    # -- pcl::Registration setters -----------------------------------------------------------
    def setMaximumIterations(self, n: int):
        self.params.max_iter = int(n)
        self._push_params()

    def getMaximumIterations(self) -> int:
        return int(self.params.max_iter)

    def setMaxCorrespondenceDistance(self, d: float):
        self.params.max_corr_dist = float(d)
        self._push_params()

    def setTransformationEpsilon(self, eps: float):
        self.params.tf_eps = float(eps)
        self._push_params()

    def setRotationEpsilon(self, eps: float):
        self.params.rot_eps = float(eps)
        self._push_params()

    # -- pcl::GeneralizedIterativeClosestPoint setters ----------------------------------------
    def setCorrespondenceRandomness(self, k: int):
        """k_correspondences_: the neighbours of a point's covariance (both clouds' are recomputed)"""
        self.params.k = int(k)
        self._push_params()

    def setMaximumOptimizerIterations(self, n: int):
        """max_inner_iterations_: the BFGS steps (GN: the solves) of one outer iteration"""
        self.params.max_inner_iter = int(n)
        self._push_params()

    def setGicpEpsilon(self, eps: float):
        """gicp_epsilon_: the smallest singular value of every covariance (both clouds' are recomputed)"""
        self.params.gicp_eps = float(eps)
        self._push_params()

    def setSolver(self, solver: int):
        """MGICP_SOLVER_PCL_BFGS (default, PCL 1.8.1 trajectory) or MGICP_SOLVER_GN (fast mode).
        Grids and covariances stay cached (PCL's dirty-flag semantics)."""
        self.params.solver = int(solver)
        self._push_params()

    def setRANSACOutlierRejectionThreshold(self, th: float):
        self.ransac_outlier_threshold = float(th)  # stored; GICP never uses it (PCL 1.8.1)

    def setInputSource(self, cloud):
        self._input = cloud
        keep, ptr, n, stride = self._cloud_arg(cloud)
        self._check(self._lib.mgicp_set_source(self._h, ptr, n, stride), "setInputSource")

    def setInputTarget(self, cloud):
        keep, ptr, n, stride = self._cloud_arg(cloud)
        self._check(self._lib.mgicp_set_target(self._h, ptr, n, stride), "setInputTarget")

    @staticmethod
    def _cloud_arg(cloud):
        """(owner, pointer, n, stride); `owner` keeps a converted copy alive across the call."""
        if isinstance(cloud, PointCloudRGB):
            return (cloud,) + cloud.ctypes_xyz()
        a = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
        return a, a.ctypes.data, len(a), 12

    def set_source_xyz(self, xyz):
        self._src_keep = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._input = None
        self._check(self._lib.mgicp_set_source(self._h, self._src_keep.ctypes.data, len(self._src_keep), 12),
                    "set_source")

    def set_target_xyz(self, xyz):
        self._tgt_keep = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._check(self._lib.mgicp_set_target(self._h, self._tgt_keep.ctypes.data, len(self._tgt_keep), 12),
                    "set_target")

    def set_source_device(self, ptr: int, n: int, stride: int):
        self._input = None
        self._check(self._lib.mgicp_set_source_device(self._h, ctypes.c_void_p(ptr), n, stride), "set_source_device")

    def set_target_device(self, ptr: int, n: int, stride: int):
        self._check(self._lib.mgicp_set_target_device(self._h, ctypes.c_void_p(ptr), n, stride), "set_target_device")

    # -- the hot path ----------------------------------------------------------------------
    def align(self, output: PointCloudRGB | None = None, guess=None) -> np.ndarray:
        """Registration::align(output, guess).  Returns getFinalTransformation()."""
        g = _cm(guess) if guess is not None else None
        out = np.zeros(16, np.float32)
        res = _lib.MgicpResult()
        rc = self._lib.mgicp_align(self._h, _fp(g) if g is not None else None, _fp(out), ctypes.byref(res))
        self.last_result = {k: getattr(res, k) for k, _ in _lib.MgicpResult._fields_}
        if rc == _lib.MGICP_E_SOLVER:
            self._converged = False  # PCL catches the solver exception; converged_ stays false
        else:
            self._check(rc, "align")
            self._converged = bool(res.converged)
        self._final = _from_cm(out)
        if output is not None and isinstance(self._input, PointCloudRGB):
            # output = transformPointCloud(*input_, output, final_transformation_)
            output.copy_from(self._input)
            self.transform_source_into(self._final, output)
        return self._final

    def hasConverged(self) -> bool:
        return self._converged

    def getFinalTransformation(self) -> np.ndarray:
        return self._final.copy()

    def getFitnessScore(self, max_range: float = DBL_MAX) -> float:
        out = ctypes.c_double()
        self._check(self._lib.mgicp_fitness(self._h, _fp(_cm(self._final)), max_range, ctypes.byref(out)),
                    "getFitnessScore")
        return out.value

    def fitness(self, T, max_range: float = DBL_MAX) -> float:
        out = ctypes.c_double()
        self._check(self._lib.mgicp_fitness(self._h, _fp(_cm(T)), max_range, ctypes.byref(out)), "fitness")
        return out.value

    def transform_source_into(self, T, cloud: PointCloudRGB):
        """xyz of `cloud` := T * source (device kernel; `cloud` must have the source's size)."""
        ptr, n, stride = cloud.ctypes_xyz()
        self._check(self._lib.mgicp_transform_source(self._h, _fp(_cm(T)), ctypes.c_void_p(ptr), stride),
                    "transform_source")

    def transform_cloud(self, T, cloud_in: PointCloudRGB, cloud_out: PointCloudRGB) -> None:
        """pcl::transformPointCloud(cloud_in, cloud_out, T) with the xyz transform on the GPU."""
        if cloud_out is not cloud_in:
            cloud_out.copy_from(cloud_in)
        _, ptr, n, stride = self._cloud_arg(cloud_out)
        self._check(self._lib.mgicp_transform_cloud(self._h, _fp(_cm(T)), ctypes.c_void_p(ptr), n, stride,
                                                    ctypes.c_void_p(ptr), stride), "transform_cloud")

    # -- helpers of GICPAlignment(use_covariances=true) --------------------------------------
    def cloud_resolution(self, cloud) -> float:
        """Utils::computeCloudResolution on the GPU (mean distance to the nearest other point)."""
        keep, ptr, n, stride = self._cloud_arg(cloud)
        out = ctypes.c_double()
        self._check(self._lib.mgicp_cloud_resolution(self._h, ctypes.c_void_p(ptr), n, stride, ctypes.byref(out)),
                    "cloud_resolution")
        return out.value

    def radius_filter(self, cloud, radius: float, min_neighbors: int = 3) -> np.ndarray:
        """bool mask: >= min_neighbors points (self included) within `radius` (NormalEstimation's
        non-NaN condition)."""
        keep, ptr, n, stride = self._cloud_arg(cloud)
        keep = np.zeros(n, np.uint8)
        self._check(self._lib.mgicp_radius_filter(self._h, ctypes.c_void_p(ptr), n, stride, float(radius),
                                                  int(min_neighbors), keep.ctypes.data), "radius_filter")
        return keep.astype(bool)

    def estimate_normals(self, cloud, radius: float, viewpoint=None):
        """pcl::NormalEstimation with a radius search (Utils::getNormals): (normals float32[n, 3],
        curvature float32[n], n_neighbors int32[n], info).  A non-finite record or one with fewer than
        3 radius neighbours (itself included) has a NaN normal and curvature; `viewpoint` None is
        PCL's default (0, 0, 0)."""
        _keep, ptr, n, stride = self._cloud_arg(cloud)
        normals = np.zeros((max(n, 1), 3), np.float32)
        curvature = np.zeros(max(n, 1), np.float32)
        count = np.zeros(max(n, 1), np.int32)
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(3)
        ni = _lib.MgicpNormalsInfo()
        self._check(self._lib.mgicp_estimate_normals(
            self._h, ctypes.c_void_p(ptr), n, stride, float(radius), _fp(vp) if vp is not None else None,
            normals.ctypes.data, 12, curvature.ctypes.data, count.ctypes.data, ctypes.byref(ni)), "estimate_normals")
        info = {f: getattr(ni, f) for f, _ in ni._fields_}
        return normals[:n], curvature[:n], count[:n], info

    def boundary_points(self, cloud, normals, k: int = 30, angle_threshold: float = 1.047, want_gap: bool = False,
                        want_indices: bool = False):
        """pcl::BoundaryEstimation with a k-search (InitialAlignment::obtainBoundaryKeypoints): (boundary
        bool[n], max_gap float32[n] | None, nn_indices int32[n, k] | None, info).  `normals` is float32
        [n, 3] or [n, 4] (as getNormals returns it), one per record of `cloud`.  A non-finite record, a
        record with a non-finite normal or a set without three members or without an angle is never a
        boundary point (max_gap NaN)."""
        _keep, ptr, n, stride = self._cloud_arg(cloud)
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] < 3 or len(nrm) != n:
            raise ValueError(f"normals must be [{n}, 3] or [{n}, 4], got {nrm.shape}")
        k = int(k)
        flags = np.zeros(max(n, 1), np.uint8)
        gap = np.zeros(max(n, 1), np.float32) if want_gap else None
        nn = np.zeros((max(n, 1), max(k, 1)), np.int32) if want_indices else None
        bi = _lib.MgicpBoundaryInfo()
        self._check(self._lib.mgicp_boundary_points(
            self._h, ctypes.c_void_p(ptr), n, stride, ctypes.c_void_p(nrm.ctypes.data), 4 * nrm.shape[1], k,
            float(angle_threshold), flags.ctypes.data, gap.ctypes.data if want_gap else None,
            nn.ctypes.data if want_indices else None, ctypes.byref(bi)), "boundary_points")
        info = {f: getattr(bi, f) for f, _ in bi._fields_}
        return (flags[:n].astype(bool), gap[:n] if want_gap else None, nn[:n] if want_indices else None, info)

    def harris_keypoints(self, cloud, normals, radius: float, threshold: float = 1e-6, nonmax: bool = True,
                         want_response: bool = False, want_covar: bool = False, want_counts: bool = False):
        """pcl::HarrisKeypoint3D (method HARRIS) with a radius search (InitialAlignment::obtainHarrisKeypoints):
        (keypoints int32[nk] ascending, response float32[n] | None, covar float32[n, 6] | None, n_neighbors
        int32[n] | None, info).  `normals` is float32 [n, 3] or [n, 4], one per record of `cloud`.  A keypoint
        is a finite record with a finite response not below float32(threshold) that no record within the
        radius exceeds; nonmax False lists every record, as PCL's branch does."""
        _keep, ptr, n, stride = self._cloud_arg(cloud)
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] < 3 or len(nrm) != n:
            raise ValueError(f"normals must be [{n}, 3] or [{n}, 4], got {nrm.shape}")
        kp = np.full(max(n, 1), -1, np.int32)
        resp = np.zeros(max(n, 1), np.float32) if want_response else None
        cov = np.zeros((max(n, 1), 6), np.float32) if want_covar else None
        cnt = np.zeros(max(n, 1), np.int32) if want_counts else None
        nk = ctypes.c_size_t()
        hi = _lib.MgicpHarrisInfo()
        self._check(self._lib.mgicp_harris_keypoints(
            self._h, ctypes.c_void_p(ptr), n, stride, ctypes.c_void_p(nrm.ctypes.data), 4 * nrm.shape[1],
            float(radius), float(np.float32(threshold)), 1 if nonmax else 0, kp.ctypes.data, ctypes.byref(nk),
            resp.ctypes.data if want_response else None, cov.ctypes.data if want_covar else None,
            cnt.ctypes.data if want_counts else None, ctypes.byref(hi)), "harris_keypoints")
        info = {f: getattr(hi, f) for f, _ in hi._fields_}
        return (kp[:nk.value].copy(), resp[:n] if want_response else None, cov[:n] if want_covar else None,
                cnt[:n] if want_counts else None, info)

    def fpfh_features(self, cloud, normals, keypoints=None, radius: float = 0.0, want_spfh: bool = False):
        """pcl::FPFHEstimation with a radius search (InitialAlignment::obtainFeatures): (fpfh float32
        [nk, 33], spfh_counts uint16[n, 33] | None, spfh_sizes int32[n] | None, info).  `normals` is float32
        [n, 3] or [n, 4], one per record of `cloud`; `keypoints` are record indices in any order, repeats
        allowed (None: every record).  Row k is the histogram of keypoints[k]: NaN for a non-finite record,
        zeros for a record alone in its radius.  With want_spfh, the SPFH bin counts and set sizes of the
        records within the radius of some keypoint (zero elsewhere)."""
        _keep, ptr, n, stride = self._cloud_arg(cloud)
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] < 3 or len(nrm) != n:
            raise ValueError(f"normals must be [{n}, 3] or [{n}, 4], got {nrm.shape}")
        kp = None if keypoints is None else np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1)
        nk = n if kp is None else len(kp)
        fpfh = np.zeros((max(nk, 1), 33), np.float32)
        counts = np.zeros((max(n, 1), 33), np.uint16) if want_spfh else None
        sizes = np.zeros(max(n, 1), np.int32) if want_spfh else None
        fi = _lib.MgicpFpfhInfo()
        self._check(self._lib.mgicp_fpfh_features(
            self._h, ctypes.c_void_p(ptr), n, stride, ctypes.c_void_p(nrm.ctypes.data), 4 * nrm.shape[1],
            ctypes.c_void_p(kp.ctypes.data) if kp is not None else None, nk, float(radius), fpfh.ctypes.data, 132,
            counts.ctypes.data if want_spfh else None, sizes.ctypes.data if want_spfh else None, ctypes.byref(fi)),
            "fpfh_features")
        info = {f: getattr(fi, f) for f, _ in fi._fields_}
        return (fpfh[:nk], counts[:n] if want_spfh else None, sizes[:n] if want_spfh else None, info)

    @staticmethod
    def _feature_arg(features, what: str):
        """(keepalive array, n, stride in bytes) of float32 rows of at least 33 values"""
        f = np.asarray(features)
        if f.ndim != 2 or f.shape[1] < 33:
            raise ValueError(f"{what} must be [n, 33] (or wider rows), got {f.shape}")
        f = np.ascontiguousarray(f, dtype=np.float32)
        return f, len(f), 4 * f.shape[1]

    def match_features(self, source_features, target_features, max_distance: float | None = None):
        """pcl::registration::CorrespondenceEstimation::determineCorrespondences over FPFHSignature33
        (InitialAlignment::obtainCorrespondences): (match int32[ns], distance float32[ns], info).  The inputs are
        float32 [n, 33], or wider rows whose first 33 values are the descriptor (passed with their stride).
        match[i] is the target row with the smallest float squared distance to source row i (equal distances:
        the lowest row), distance[i] that squared distance; -1 and NaN for a source row with a non-finite
        value, without a finite target row, or farther than max_distance (None: DBL_MAX, nothing rejected)."""
        src, ns, sstride = self._feature_arg(source_features, "source_features")
        tgt, nt, tstride = self._feature_arg(target_features, "target_features")
        match = np.full(max(ns, 1), -1, np.int32)
        dist = np.full(max(ns, 1), np.nan, np.float32)
        cnt = ctypes.c_size_t()
        mi = _lib.MgicpMatchInfo()
        self._check(self._lib.mgicp_match_features(
            self._h, ctypes.c_void_p(src.ctypes.data) if ns else None, ns, sstride,
            ctypes.c_void_p(tgt.ctypes.data) if nt else None, nt, tstride,
            float(np.finfo(np.float64).max) if max_distance is None else float(max_distance),
            match.ctypes.data, dist.ctypes.data, ctypes.byref(cnt), ctypes.byref(mi)), "match_features")
        info = {f: getattr(mi, f) for f, _ in mi._fields_}
        return match[:ns], dist[:ns], info

    # -- the pre-alignment transform: the rejectors and the SVD estimate -------------------------
    @staticmethod
    def _keypoint_arg(cloud):
        """(owner, pointer or None, n, stride) of a keypoint cloud: a PointCloudRGB, or float32 rows of at least
        3 values whose first 3 are x, y, z (passed with their stride)"""
        if isinstance(cloud, PointCloudRGB):
            _p, n, stride = cloud.ctypes_xyz()
            return cloud, ctypes.c_void_p(_p) if n else None, n, stride
        a = np.asarray(cloud)
        if a.ndim != 2 or a.shape[1] < 3:
            a = a.reshape(-1, 3)
        a = np.ascontiguousarray(a, dtype=np.float32)
        return a, ctypes.c_void_p(a.ctypes.data) if len(a) else None, len(a), 4 * a.shape[1]

    @staticmethod
    def _index_arg(idx, m=None):
        a = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        if m is not None and len(a) != m:
            raise ValueError(f"the correspondence arrays differ in length: {len(a)} and {m}")
        return a

    def _pair_args(self, source_keypoints, target_keypoints, index_query, index_match):
        sk, sp, ns, ss = self._keypoint_arg(source_keypoints)
        tk, tp, nt, ts = self._keypoint_arg(target_keypoints)
        iq = self._index_arg(index_query)
        im = self._index_arg(index_match, len(iq))
        m = len(iq)
        return (sk, tk, iq, im), (sp, ns, ss, tp, nt, ts, ctypes.c_void_p(iq.ctypes.data) if m else None,
                                  ctypes.c_void_p(im.ctypes.data) if m else None, m)

    def reject_ransac(self, source_keypoints, target_keypoints, index_query, index_match,
                      inlier_threshold: float = 1.5, max_iterations: int = 1000, refine: bool = True):
        """pcl::registration::CorrespondenceRejectorSampleConsensus (InitialAlignment::rejectCorrespondences):
        (keep bool[m], best_T float32[4, 4], info).  The remaining correspondences are those with keep, in
        input order; everything is kept and best_T is the identity when PCL returns its input (no model, a
        failed refine, fewer than 3 inliers)."""
        _alive, args = self._pair_args(source_keypoints, target_keypoints, index_query, index_match)
        m = args[-1]
        keep = np.zeros(max(m, 1), np.uint8)
        cnt = ctypes.c_size_t()
        T = np.zeros(16, np.float32)
        ri = _lib.MgicpRansacInfo()
        self._check(self._lib.mgicp_reject_ransac(self._h, *args, float(inlier_threshold), int(max_iterations),
                                                  int(bool(refine)), keep.ctypes.data, ctypes.byref(cnt), _fp(T),
                                                  ctypes.byref(ri)), "reject_ransac")
        info = {f: getattr(ri, f) for f, _ in ri._fields_}
        info["n_keep"] = int(cnt.value)
        return keep[:m].astype(bool), _from_cm(T), info

    def reject_one_to_one(self, index_match, distance, n_target: int):
        """pcl::registration::CorrespondenceRejectorOneToOne (InitialAlignment::rejectOneToOneCorrespondences):
        (order int32[n_keep], info) -- the positions of the surviving correspondences in ascending index_match:
        per target the smallest distance, equal distances the lowest position."""
        im = self._index_arg(index_match)
        m = len(im)
        d = np.ascontiguousarray(distance, dtype=np.float32).reshape(-1)
        if len(d) != m:
            raise ValueError(f"the correspondence arrays differ in length: {len(d)} and {m}")
        order = np.full(max(m, 1), -1, np.int32)
        cnt = ctypes.c_size_t()
        ms = ctypes.c_double()
        self._check(self._lib.mgicp_reject_one_to_one(
            self._h, ctypes.c_void_p(im.ctypes.data) if m else None, ctypes.c_void_p(d.ctypes.data) if m else None, m,
            int(n_target), order.ctypes.data, ctypes.byref(cnt), ctypes.byref(ms)), "reject_one_to_one")
        assert (order[int(cnt.value):m] == -1).all()
        return order[:int(cnt.value)].copy(), {"n_keep": int(cnt.value), "ms_device": ms.value}

    def estimate_rigid_svd(self, source_keypoints, target_keypoints, index_query, index_match):
        """pcl::registration::TransformationEstimationSVD (InitialAlignment::estimateTransform) over the
        correspondences: (T float32[4, 4], info); info["sums"] are the 15 raw fp64 sums."""
        _alive, args = self._pair_args(source_keypoints, target_keypoints, index_query, index_match)
        T = np.zeros(16, np.float32)
        si = _lib.MgicpSvdInfo()
        self._check(self._lib.mgicp_estimate_rigid_svd(self._h, *args, _fp(T), ctypes.byref(si)), "estimate_rigid_svd")
        return _from_cm(T), {"sums": np.array(si.sums[:], np.float64), "ms_device": si.ms_device,
                             "ms_total": si.ms_total}

    def debug_score_models(self, source_keypoints, target_keypoints, index_query, index_match, models, threshold):
        """mgicp_debug_score_models: the inlier count of each [4, 4] model in `models` ([B, 4, 4])"""
        _alive, args = self._pair_args(source_keypoints, target_keypoints, index_query, index_match)
        mod = np.asarray(models, dtype=np.float32).reshape(-1, 4, 4)
        cm = np.ascontiguousarray(mod.transpose(0, 2, 1)).reshape(-1)
        counts = np.zeros(max(len(mod), 1), np.int32)
        self._check(self._lib.mgicp_debug_score_models(
            self._h, *args, ctypes.c_void_p(cm.ctypes.data) if len(mod) else None, len(mod), float(threshold),
            counts.ctypes.data), "debug_score_models")
        return counts[:len(mod)]

    # -- FOD-side callers ------------------------------------------
    def segment_differences(self, cloud_in, cloud_sub, sqr_threshold: float, T=None):
        """pcl::SegmentDifferences (Filter::removeFromCloud): bool keep mask over cloud_in (after T)
        and the kept count."""
        keep_in, pin, n, sin_ = self._cloud_arg(cloud_in)
        keep_sub, psub, ns, ssub = self._cloud_arg(cloud_sub)
        keep = np.zeros(max(n, 1), np.uint8)
        cnt = ctypes.c_size_t()
        tcm = _cm(T) if T is not None else None
        self._check(self._lib.mgicp_segment_differences(
            self._h, _fp(tcm) if tcm is not None else None, ctypes.c_void_p(pin), n, sin_, ctypes.c_void_p(psub),
            ns, ssub, float(sqr_threshold), keep.ctypes.data, ctypes.byref(cnt)), "segment_differences")
        return keep[:n].astype(bool), int(cnt.value)

    def euclidean_clusters(self, cloud, tolerance: float, min_size: int = 1, max_size: int = 0):
        """pcl::EuclideanClusterExtraction (FODDetector::clusterPossibleFODs): (clusters, labels, info).
        `clusters`: int32 index arrays, largest first (equal sizes by smallest member), members
        ascending; `labels`: per record the rank of its cluster or -1; `info`: the call's counters."""
        min_size, max_size = int(min_size), int(max_size)
        if min_size < 0 or max_size < 0:  # would wrap to a huge size_t
            raise ValueError(f"euclidean_clusters: min_size {min_size} / max_size {max_size} must be >= 0")
        _keep, ptr, n, stride = self._cloud_arg(cloud)
        labels = np.full(max(n, 1), -1, np.int32)
        indices = np.zeros(max(n, 1), np.int32)
        offsets = np.zeros(n + 1, np.uintp)
        ci = _lib.MgicpClusterInfo()
        self._check(self._lib.mgicp_euclidean_clusters(
            self._h, ctypes.c_void_p(ptr), n, stride, float(tolerance), int(min_size), int(max_size),
            labels.ctypes.data, indices.ctypes.data, offsets.ctypes.data, ctypes.byref(ci)), "euclidean_clusters")
        off = offsets.astype(np.int64)
        clusters = [indices[off[c]:off[c + 1]].copy() for c in range(ci.n_clusters)]
        info = {f: getattr(ci, f) for f, _ in ci._fields_}
        info["offsets"] = off[:ci.n_clusters + 1]
        return clusters, labels[:n], info

    def normal_clusters(self, cloud, normals, tolerance: float, eps_angle: float, min_size: int = 1, max_size: int = 0):
        """pcl::extractEuclideanClusters with normals (InitialAlignment::obtainNormalsCluster): (clusters,
        labels, info).  PCL's serial rounds in ascending seed: a round takes what its seed reaches by links
        through unprocessed records whose normal is within eps_angle of the SEED's.  `clusters`: int32 index
        arrays in ascending seed, members ascending; `labels`: per record the rank of its cluster or -1;
        `normals` is float32 [n, 3] or [n, 4], one per record of `cloud`."""
        min_size, max_size = int(min_size), int(max_size)
        if min_size < 0 or max_size < 0:  # would wrap to a huge size_t
            raise ValueError(f"normal_clusters: min_size {min_size} / max_size {max_size} must be >= 0")
        _keep, ptr, n, stride = self._cloud_arg(cloud)
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] < 3 or len(nrm) != n:
            raise ValueError(f"normals must be [{n}, 3] or [{n}, 4], got {nrm.shape}")
        labels = np.full(max(n, 1), -1, np.int32)
        indices = np.zeros(max(n, 1), np.int32)
        offsets = np.zeros(n + 1, np.uintp)
        ci = _lib.MgicpNormalClusterInfo()
        self._check(self._lib.mgicp_normal_clusters(
            self._h, ctypes.c_void_p(ptr), n, stride, ctypes.c_void_p(nrm.ctypes.data), 4 * nrm.shape[1],
            float(tolerance), float(eps_angle), min_size, max_size, labels.ctypes.data, indices.ctypes.data,
            offsets.ctypes.data, ctypes.byref(ci)), "normal_clusters")
        off = offsets.astype(np.int64)
        nc = int(ci.n_clusters)
        clusters = [indices[off[c]:off[c + 1]].copy() for c in range(nc)]
        info = {f: getattr(ci, f) for f, _ in ci._fields_}
        info["offsets"] = off[:nc + 1]
        return clusters, labels[:n], info

    def dominant_normals(self, normals, clusters):
        """InitialAlignment::obtainDominantNormals: float32 [len(clusters), 3], per cluster the normalised sum of
        its members' normals with the first member counted twice (as the reference does).  `clusters`: index
        arrays into `normals` (float32 [n, 3] or [n, 4]).  The call's device time lands in last_dominant_ms."""
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] < 3:
            raise ValueError(f"normals must be [n, 3] or [n, 4], got {nrm.shape}")
        members = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in clusters]
        nc = len(members)
        indices = np.concatenate(members).astype(np.int32) if nc else np.zeros(0, np.int32)
        offsets = np.zeros(nc + 1, np.uintp)
        offsets[1:] = np.cumsum([len(m) for m in members])
        out = np.zeros((max(nc, 1), 3), np.float32)
        ms = ctypes.c_double()
        self._check(self._lib.mgicp_dominant_normals(
            self._h, ctypes.c_void_p(nrm.ctypes.data), len(nrm), 4 * nrm.shape[1], ctypes.c_void_p(indices.ctypes.data),
            offsets.ctypes.data, nc, out.ctypes.data, ctypes.byref(ms)), "dominant_normals")
        self.last_dominant_ms = ms.value
        return out[:nc]

    def voxel_grid(self, cloud: PointCloudRGB, leaf, min_points_per_voxel: int = 0) -> PointCloudRGB:
        """pcl::VoxelGrid<PointXYZRGB>::filter (Filter::downsampleCloud) -> a new cloud."""
        from .cloud import POINT_XYZRGB

        leaf = np.broadcast_to(np.asarray(leaf, np.float64), (3,)).copy()
        _, ptr, n, stride = self._cloud_arg(cloud)
        out = PointCloudRGB()
        out.points = np.empty(max(n, 1), dtype=POINT_XYZRGB)  # capacity; the call writes n_out whole records
        nout = ctypes.c_size_t()
        self._check(self._lib.mgicp_voxel_grid(
            self._h, ctypes.c_void_p(ptr), n, stride, int(POINT_XYZRGB.fields["rgb"][1]), _dp(leaf),
            int(min_points_per_voxel), out.points.ctypes.data, POINT_XYZRGB.itemsize, ctypes.byref(nout)),
            "voxel_grid")
        out.points = out.points[:nout.value].copy()
        return out

    # -- multi-GPU ------------------------------------------------------------------------
    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        rc = _lib.load().mgicp_get_unique_id(buf)
        if rc != 0:
            raise _lib.MgicpError(rc, "mgicp_get_unique_id")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes | None):
        buf = ctypes.create_string_buffer(uid, 128) if uid is not None else None
        self._check(self._lib.mgicp_comm_init(self._h, nranks, rank, buf), "comm_init")

    def attach_shm(self, name: str, max_source_points: int = 0):
        """Node-local transport of the per-pass sums (every rank, same name): the GPUs write their
        super rows into one shared-memory segment, every host takes the same fixed-order total."""
        self._check(self._lib.mgicp_comm_attach_shm(self._h, name.encode(), int(max_source_points)),
                    "comm_attach_shm")

    def attach_xgmi(self, on: bool = True):
        """per-pass super rows over xGMI (peer device memory) after attach_shm (mgicp_comm_attach_xgmi)"""
        self._check(self._lib.mgicp_comm_attach_xgmi(self._h, int(bool(on))), "mgicp_comm_attach_xgmi")

    def detach_shm(self):
        """Back to the previous transport (RCCL or local)."""
        self._check(self._lib.mgicp_comm_attach_shm(self._h, None, 0), "comm_attach_shm(detach)")

    PASS_STATS = ("server_launches", "server_passes", "launched_passes", "takeovers", "bar_commands",
                  "row_allocs", "transport", "server_denied", "memo_hits")

    def pass_stats(self) -> dict:
        """Objective-pass path counters (mgicp_debug_pass_stats)."""
        out = (ctypes.c_longlong * len(self.PASS_STATS))()
        self._check(self._lib.mgicp_debug_pass_stats(self._h, out), "pass_stats")
        return {k: int(out[i]) for i, k in enumerate(self.PASS_STATS)}

    ROUND_STATS = ("fast", "slow", "deferred", "pending")

    def round_stats(self) -> dict:
        """Correspondence rounds of the BFGS mode (mgicp_debug_round_stats)."""
        out = (ctypes.c_longlong * len(self.ROUND_STATS))()
        self._check(self._lib.mgicp_debug_round_stats(self._h, out), "round_stats")
        return {k: int(out[i]) for i, k in enumerate(self.ROUND_STATS)}

    def server_time(self, reset: bool = False) -> dict:
        """The resident pass server as the aligns run it (mgicp_debug_server_time): summed launch
        duration, passes and launches since the last reset; ms_per_pass = the in-align pass."""
        ms = ctypes.c_double()
        passes = ctypes.c_longlong()
        launches = ctypes.c_longlong()
        self._check(self._lib.mgicp_debug_server_time(self._h, ctypes.byref(ms), ctypes.byref(passes),
                                                      ctypes.byref(launches), int(reset)), "server_time")
        p = int(passes.value)
        return {"ms": ms.value, "passes": p, "launches": int(launches.value),
                "ms_per_pass": ms.value / p if p else None}

    def debug_target_cov_slice(self, nranks: int, rank: int, n_target: int) -> np.ndarray:
        """slice `rank` of `nranks` of the target covariances as an N-rank context computes it before
        its all-gather (mgicp_debug_target_cov_slice)"""
        out = np.zeros((max(1, -(-n_target // nranks)), 6), np.float64)
        cnt = self._check(self._lib.mgicp_debug_target_cov_slice(self._h, int(nranks), int(rank), _dp(out)),
                          "debug_target_cov_slice")
        return out[:cnt].copy()

    MATCH_STATS = ("pairs", "left_after_8", "left_after_16", "left_after_24", "launches", "rows_per_launch",
                   "splits", "rows_per_split")

    def match_stats(self) -> dict:
        """The last match_features call of this engine (mgicp_debug_match_stats)."""
        out = (ctypes.c_longlong * 8)()
        self._check(self._lib.mgicp_debug_match_stats(self._h, out), "match_stats")
        return {k: int(out[i]) for i, k in enumerate(self.MATCH_STATS)}

    VLIST_STATS = ("requested", "pending", "lists", "entries", "reject", "overflow", "pool_used", "cells")

    def vlist_stats(self) -> dict:
        """The target's 1-NN cell lists (mgicp_debug_vlist_stats)."""
        out = (ctypes.c_longlong * 8)()
        self._check(self._lib.mgicp_debug_vlist_stats(self._h, out), "vlist_stats")
        return {k: int(out[i]) for i, k in enumerate(self.VLIST_STATS)}

    VLIST_LAYOUT = ("ox", "oy", "oz", "c", "es", "nx", "ny", "nz", "gate", "h", "vl_off", "pool_cap", "pool_head",
                    "build_cap", "requested", "pending", "second_pass", "cells", "allocated", "inv_c")
    VLIST_STATES = ("not_built", "touched", "requested", "reject", "overflow", "listed")

    def vlist_layout(self, cells: bool = False):
        """The fine grid of the 1-NN cell lists and its counters (mgicp_debug_vlist_layout) as a dict; with
        cells = True also (state, length, offset): per fine cell its class (index into VLIST_STATES), its
        list's true length and first pool entry (None when nothing is allocated).  cells = "state": the
        classes alone, (state, None, None) -- one byte per cell, for grids of 2^28 cells."""
        out = np.zeros(24, np.float64)
        self._check(self._lib.mgicp_debug_vlist_layout(self._h, _dp(out), None, None, None, 0), "vlist_layout")
        ints = ("nx", "ny", "nz", "vl_off", "pool_cap", "pool_head", "build_cap", "requested", "pending",
                "second_pass", "cells", "allocated")
        lay = {k: (int(out[i]) if k in ints else float(out[i])) for i, k in enumerate(self.VLIST_LAYOUT)}
        if not cells:
            return lay
        if not lay["allocated"]:
            return lay, None
        n = lay["cells"]
        state = np.zeros(n, np.uint8)
        length = offset = None
        if cells != "state":
            length = np.zeros(n, np.uint32)
            offset = np.zeros(n, np.uint32)
        self._check(self._lib.mgicp_debug_vlist_layout(
            self._h, _dp(out), state.ctypes.data, None if length is None else length.ctypes.data,
            None if offset is None else offset.ctypes.data, n), "vlist_layout")
        for i, k in enumerate(self.VLIST_LAYOUT):
            lay[k] = int(out[i]) if k in ints else float(out[i])
        return lay, (state, length, offset)

    # -- introspection (parity tests, profiling) ----------------------------------------------
    def debug_source_order(self, n: int) -> np.ndarray:
        """Original indices of the source points in the objective's stream order (mgicp_debug_source_order)."""
        out = np.zeros(n, np.uint32)
        m = self._check(self._lib.mgicp_debug_source_order(self._h, out.ctypes.data, n), "debug_source_order")
        return out[:m]

    def debug_covariances(self, which: str, n: int) -> np.ndarray:
        out = np.zeros((n, 6), np.float64)
        self._check(self._lib.mgicp_debug_covariances(self._h, 0 if which == "source" else 1, _dp(out)),
                    "debug_covariances")
        return out

    def debug_correspondences(self, T, n: int):
        tgt = np.full(n, -1, np.int32)
        M = np.zeros((n, 6), np.float64)
        m = self._check(self._lib.mgicp_debug_correspondences(
            self._h, _fp(_cm(T)), tgt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(M)), "debug_correspondences")
        return m, tgt, M

    def debug_correspondences_seeded(self, T, n: int):
        """The same sweep seeded with the previous sweep's matches (outer iterations >= 2)."""
        tgt = np.full(n, -1, np.int32)
        M = np.zeros((n, 6), np.float64)
        m = self._check(self._lib.mgicp_debug_correspondences_seeded(
            self._h, _fp(_cm(T)), tgt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(M)),
            "debug_correspondences_seeded")
        return m, tgt, M

    def debug_fdf(self, x):
        x = np.asarray(x, np.float64)
        f = ctypes.c_double()
        g = np.zeros(6, np.float64)
        self._check(self._lib.mgicp_debug_fdf(self._h, _dp(x), ctypes.byref(f), _dp(g)), "debug_fdf")
        return f.value, g

    def debug_fdf_sums(self, x) -> np.ndarray:
        x = np.asarray(x, np.float64)
        out = np.zeros(16, np.float64)
        self._check(self._lib.mgicp_debug_fdf_sums(self._h, _dp(x), _dp(out)), "debug_fdf_sums")
        return out

    def debug_fdf_sums_run(self, xs) -> np.ndarray:
        """(n, 16) sums of n passes at the states xs (n, 6) run as one BFGS run makes them: one live
        server for all of them (mgicp_debug_fdf_sums_run)"""
        xs = np.ascontiguousarray(np.asarray(xs, np.float64).reshape(-1, 6))
        out = np.zeros((len(xs), 16), np.float64)
        self._check(self._lib.mgicp_debug_fdf_sums_run(self._h, _dp(xs), len(xs), _dp(out)), "debug_fdf_sums_run")
        return out

    def debug_wave_reduce(self, vals) -> tuple:
        """(shuffle-tree sums, reduce-scatter sums) of vals[w][64][16] per wave w (the chunk reduction)"""
        vals = np.ascontiguousarray(vals, np.float64)
        nw = vals.shape[0]
        assert vals.shape == (nw, 64, 16)
        tree = np.zeros((nw, 16), np.float64)
        rs = np.zeros((nw, 16), np.float64)
        self._check(self._lib.mgicp_debug_wave_reduce(self._h, _dp(vals), int(nw), _dp(tree), _dp(rs)),
                    "debug_wave_reduce")
        return tree, rs

    def debug_pass_bench(self, x, npasses: int, mode: int = 0):
        """(ms per pass, sums of the last pass): npasses objective passes at x over the last sweep,
        back to back (mode 0: the resident pass server, 1: one launch per pass), HIP-event timed"""
        x = np.asarray(x, np.float64)
        ms = ctypes.c_double()
        out = np.zeros(16, np.float64)
        self._check(self._lib.mgicp_debug_pass_bench(self._h, _dp(x), int(npasses), int(mode), ctypes.byref(ms),
                                                     _dp(out)), "debug_pass_bench")
        return ms.value, out

    def debug_trace(self, max_iters: int = 1000):
        buf = np.zeros(16 * max_iters, np.float32)
        n = self._check(self._lib.mgicp_debug_trace(self._h, _fp(buf), max_iters), "debug_trace")
        return [_from_cm(buf[16 * i:16 * i + 16]) for i in range(min(n, max_iters))]

    def set_profiling(self, on: bool):
        self._check(self._lib.mgicp_set_profiling(self._h, int(on)), "set_profiling")

    def debug_moments(self, T) -> np.ndarray:
        """MGICP_SOLVER_GN's 74 moments (+ pad) at T over the last correspondence sweep."""
        out = np.zeros(80, np.float64)
        self._check(self._lib.mgicp_debug_moments(self._h, _fp(_cm(T)), _dp(out)), "debug_moments")
        return out

    def debug_supers(self, kind: str, arg) -> np.ndarray:
        """This shard's super partials of one pass of the fixed reduction tree: kind "fdf" (arg = x),
        "moments" (arg = T) or "fitness" (arg = (T, max_range)); shape (nsup_local, 16 or 80)."""
        if kind == "fdf":
            k, a, nv = 0, np.asarray(arg, np.float64), 16
        elif kind == "moments":
            k, a, nv = 1, np.asarray(_cm(arg), np.float64), 80
        elif kind == "fitness":
            T, max_range = arg
            k, a, nv = 2, np.concatenate([np.asarray(_cm(T), np.float64), [float(max_range)]]), 16
        else:
            raise ValueError(kind)
        cap = 1 << 16
        out = np.zeros((cap, nv), np.float64)
        n = self._check(self._lib.mgicp_debug_supers(self._h, k, _dp(np.ascontiguousarray(a)), _dp(out), cap),
                        "debug_supers")
        return out[:n].copy()

    def debug_finish_supers(self, rows: np.ndarray, nsup: int, maxsup: int, nranks: int) -> np.ndarray:
        """The multi-GPU finish: fixed-order total of nsup supers held as nranks rows of maxsup."""
        rows = np.ascontiguousarray(rows, np.float64)
        nv = rows.shape[-1]
        out = np.zeros(nv, np.float64)
        self._check(self._lib.mgicp_debug_finish_supers(self._h, nv, _dp(rows), nsup, maxsup, nranks, _dp(out)),
                    "debug_finish_supers")
        return out

    def kernel_times(self):
        nf = _lib.MGICP_KERNEL_FAMILIES
        ms = np.zeros(nf, np.float64)
        cnt = np.zeros(nf, np.int32)
        self._check(self._lib.mgicp_debug_kernel_times(self._h, _dp(ms), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int))),
                    "kernel_times")
        names = ["knn_cov", "correspond", "fdf", "reduce_finish", "compact", "gn_moments"]
        return {names[i]: {"avg_ms": float(ms[i]), "count": int(cnt[i])} for i in range(nf)}
