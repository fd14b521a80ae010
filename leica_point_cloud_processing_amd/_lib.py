"""ctypes binding of libmgicp.so (include/mi355x_gicp.h and, for tests and bench.py, mi355x_gicp_debug.h).

The HIP engine is the only compute path of this package: if the in-tree library is missing
or cannot be loaded, every entry point raises immediately -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("MGICP_LIB_NAME", "libmgicp.so"))  # variant builds for A/B
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mi355x_gicp.h")  # the product (drop-in) calls
DEBUG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mi355x_gicp_debug.h")  # test / bench hooks

MGICP_OK = 0
MGICP_E_INVALID = -1
MGICP_E_TOO_FEW_POINTS = -2
MGICP_E_SOLVER = -3
MGICP_E_NONFINITE = -4
MGICP_E_HIP = -5
MGICP_E_COMM = -6
MGICP_E_NOMEM = -7

MGICP_SOLVER_PCL_BFGS = 0
MGICP_SOLVER_GN = 1
MGICP_KERNEL_FAMILIES = 6


class MgicpParams(ctypes.Structure):
    _fields_ = [
        ("max_iter", ctypes.c_int),
        ("tf_eps", ctypes.c_double),
        ("rot_eps", ctypes.c_double),
        ("max_corr_dist", ctypes.c_double),
        ("gicp_eps", ctypes.c_double),
        ("k", ctypes.c_int),
        ("max_inner_iter", ctypes.c_int),
        ("solver", ctypes.c_int),
        ("device", ctypes.c_int),
        ("fixed_iterations", ctypes.c_int),
    ]


class MgicpResult(ctypes.Structure):
    _fields_ = [
        ("converged", ctypes.c_int),
        ("iterations", ctypes.c_int),
        ("n_corr", ctypes.c_int),
        ("n_evals", ctypes.c_int),
        ("ms_total", ctypes.c_double),
        ("ms_upload", ctypes.c_double),
        ("ms_prep", ctypes.c_double),
        ("ms_loop", ctypes.c_double),
    ]


class MgicpClusterInfo(ctypes.Structure):
    _fields_ = [
        ("n_clusters", ctypes.c_int),
        ("n_components", ctypes.c_int),
        ("n_clustered_points", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("ms_grid", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpNormalsInfo(ctypes.Structure):
    _fields_ = [
        ("n_finite", ctypes.c_double),
        ("n_nan", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("ms_grid", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpBoundaryInfo(ctypes.Structure):
    _fields_ = [
        ("n_finite", ctypes.c_double),
        ("n_boundary", ctypes.c_double),
        ("n_undecided", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("ms_grid", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpHarrisInfo(ctypes.Structure):
    _fields_ = [
        ("n_finite", ctypes.c_double),
        ("n_candidates", ctypes.c_double),
        ("n_keypoints", ctypes.c_double),
        ("n_tied", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("ms_grid", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpFpfhInfo(ctypes.Structure):
    _fields_ = [
        ("n_finite", ctypes.c_double),
        ("n_keypoints", ctypes.c_double),
        ("n_nan", ctypes.c_double),
        ("n_spfh_rows", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("pair_features", ctypes.c_double),
        ("ms_grid", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpMatchInfo(ctypes.Structure):
    _fields_ = [
        ("n_source_valid", ctypes.c_double),
        ("n_target_valid", ctypes.c_double),
        ("n_correspondences", ctypes.c_double),
        ("n_tied", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpRansacInfo(ctypes.Structure):
    _fields_ = [
        ("n_hypotheses", ctypes.c_double),
        ("n_iterations", ctypes.c_double),
        ("n_skipped", ctypes.c_double),
        ("n_refine_rounds", ctypes.c_double),
        ("n_inliers_ransac", ctypes.c_double),
        ("n_inliers_final", ctypes.c_double),
        ("final_error_threshold", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpSvdInfo(ctypes.Structure):
    _fields_ = [
        ("sums", ctypes.c_double * 15),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpNormalClusterInfo(ctypes.Structure):
    _fields_ = [
        ("n_rounds", ctypes.c_double),
        ("n_clusters", ctypes.c_double),
        ("n_clustered_points", ctypes.c_double),
        ("n_levels", ctypes.c_double),
        ("n_wide_rounds", ctypes.c_double),
        ("pair_tests", ctypes.c_double),
        ("ms_grid", ctypes.c_double),
        ("ms_device", ctypes.c_double),
        ("ms_total", ctypes.c_double),
    ]


class MgicpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mgicp error {code}: {msg}")
        self.code = code


_P = ctypes.c_void_p
_FP = ctypes.POINTER(ctypes.c_float)
_DP = ctypes.POINTER(ctypes.c_double)
_IP = ctypes.POINTER(ctypes.c_int)
_SZ = ctypes.c_size_t

_SIGNATURES = {
    "mgicp_default_params": (None, [ctypes.POINTER(MgicpParams)]),
    "mgicp_create": (ctypes.c_int, [ctypes.POINTER(_P), ctypes.POINTER(MgicpParams)]),
    "mgicp_set_params": (ctypes.c_int, [_P, ctypes.POINTER(MgicpParams)]),
    "mgicp_last_error": (ctypes.c_char_p, [_P]),
    "mgicp_destroy": (None, [_P]),
    "mgicp_device_count": (ctypes.c_int, [_IP]),
    "mgicp_set_target": (ctypes.c_int, [_P, _P, _SZ, _SZ]),
    "mgicp_set_source": (ctypes.c_int, [_P, _P, _SZ, _SZ]),
    "mgicp_set_target_device": (ctypes.c_int, [_P, _P, _SZ, _SZ]),
    "mgicp_set_source_device": (ctypes.c_int, [_P, _P, _SZ, _SZ]),
    "mgicp_align": (ctypes.c_int, [_P, _FP, _FP, ctypes.POINTER(MgicpResult)]),
    "mgicp_fitness": (ctypes.c_int, [_P, _FP, ctypes.c_double, _DP]),
    "mgicp_transform_source": (ctypes.c_int, [_P, _FP, _P, _SZ]),
    "mgicp_transform_cloud": (ctypes.c_int, [_P, _FP, _P, _SZ, _SZ, _P, _SZ]),
    "mgicp_cloud_resolution": (ctypes.c_int, [_P, _P, _SZ, _SZ, _DP]),
    "mgicp_radius_filter": (ctypes.c_int, [_P, _P, _SZ, _SZ, ctypes.c_double, ctypes.c_int, _P]),
    "mgicp_estimate_normals": (ctypes.c_int, [_P, _P, _SZ, _SZ, ctypes.c_double, _FP, _P, _SZ, _P, _P,
                                               ctypes.POINTER(MgicpNormalsInfo)]),
    "mgicp_boundary_points": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, ctypes.c_int, ctypes.c_double, _P, _P, _P,
                                              ctypes.POINTER(MgicpBoundaryInfo)]),
    "mgicp_harris_keypoints": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, ctypes.c_double, ctypes.c_float, ctypes.c_int,
                                               _P, ctypes.POINTER(_SZ), _P, _P, _P, ctypes.POINTER(MgicpHarrisInfo)]),
    "mgicp_fpfh_features": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _P, _SZ, ctypes.c_double, _P, _SZ, _P, _P,
                                            ctypes.POINTER(MgicpFpfhInfo)]),
    "mgicp_match_features": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, ctypes.c_double, _P, _P,
                                             ctypes.POINTER(_SZ), ctypes.POINTER(MgicpMatchInfo)]),
    "mgicp_reject_ransac": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, _SZ, ctypes.c_double, ctypes.c_int,
                                            ctypes.c_int, _P, ctypes.POINTER(_SZ), _FP,
                                            ctypes.POINTER(MgicpRansacInfo)]),
    "mgicp_reject_one_to_one": (ctypes.c_int, [_P, _P, _P, _SZ, _SZ, _P, ctypes.POINTER(_SZ), _DP]),
    "mgicp_estimate_rigid_svd": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, _SZ, _FP,
                                                 ctypes.POINTER(MgicpSvdInfo)]),
    "mgicp_normal_clusters": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, ctypes.c_double, ctypes.c_double, _SZ, _SZ, _P, _P,
                                              _P, ctypes.POINTER(MgicpNormalClusterInfo)]),
    "mgicp_dominant_normals": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _SZ, _P, _DP]),
    "mgicp_debug_score_models": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, _SZ, _P, ctypes.c_int,
                                                 ctypes.c_double, _P]),
    "mgicp_segment_differences": (ctypes.c_int, [_P, _FP, _P, _SZ, _SZ, _P, _SZ, _SZ, ctypes.c_double, _P,
                                                  ctypes.POINTER(_SZ)]),
    "mgicp_voxel_grid": (ctypes.c_int, [_P, _P, _SZ, _SZ, ctypes.c_int, _DP, ctypes.c_int, _P, _SZ,
                                         ctypes.POINTER(_SZ)]),
    "mgicp_euclidean_clusters": (ctypes.c_int, [_P, _P, _SZ, _SZ, ctypes.c_double, _SZ, _SZ, _P, _P, _P,
                                                 ctypes.POINTER(MgicpClusterInfo)]),
    "mgicp_get_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "mgicp_comm_init": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    "mgicp_comm_attach_shm": (ctypes.c_int, [_P, ctypes.c_char_p, _SZ]),
    "mgicp_comm_attach_xgmi": (ctypes.c_int, [_P, ctypes.c_int]),
    "mgicp_debug_pass_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_longlong)]),
    "mgicp_debug_round_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_longlong)]),
    "mgicp_debug_server_time": (ctypes.c_int, [_P, _DP, ctypes.POINTER(ctypes.c_longlong),
                                               ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]),
    "mgicp_debug_target_cov_slice": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _DP]),
    "mgicp_debug_vlist_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_longlong)]),
    "mgicp_debug_match_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_longlong)]),
    "mgicp_debug_vlist_layout": (ctypes.c_int, [_P, _DP, _P, _P, _P, _SZ]),
    "mgicp_debug_source_order": (ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_size_t]),
    "mgicp_debug_covariances": (ctypes.c_int, [_P, ctypes.c_int, _DP]),
    "mgicp_debug_correspondences": (ctypes.c_int, [_P, _FP, _IP, _DP]),
    "mgicp_debug_correspondences_seeded": (ctypes.c_int, [_P, _FP, _IP, _DP]),
    "mgicp_debug_fdf": (ctypes.c_int, [_P, _DP, _DP, _DP]),
    "mgicp_debug_fdf_sums": (ctypes.c_int, [_P, _DP, _DP]),
    "mgicp_debug_fdf_sums_run": (ctypes.c_int, [_P, _DP, ctypes.c_int, _DP]),
    "mgicp_debug_pass_bench": (ctypes.c_int, [_P, _DP, ctypes.c_int, ctypes.c_int, _DP, _DP]),
    "mgicp_debug_moments": (ctypes.c_int, [_P, _FP, _DP]),
    "mgicp_debug_supers": (ctypes.c_int, [_P, ctypes.c_int, _DP, _DP, ctypes.c_int]),
    "mgicp_debug_finish_supers": (ctypes.c_int, [_P, ctypes.c_int, _DP, ctypes.c_longlong, ctypes.c_longlong,
                                                 ctypes.c_int, _DP]),
    "mgicp_debug_wave_reduce": (ctypes.c_int, [_P, _DP, ctypes.c_int, _DP, _DP]),
    "mgicp_debug_trace": (ctypes.c_int, [_P, _FP, ctypes.c_int]),
    "mgicp_debug_kernel_times": (ctypes.c_int, [_P, _DP, _IP]),
    "mgicp_set_profiling": (ctypes.c_int, [_P, ctypes.c_int]),
    "mgicp_debug_option": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_double]),
    "mgicp_debug_cache_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_longlong)]),
    "mgicp_release_cache": (None, []),
}

_lib = None


def header_symbols(path: str | None = None) -> list[str]:
    """Every function one header declares; without a path, the union of the product header
    (include/mi355x_gicp.h) and the debug header (include/mi355x_gicp_debug.h): all the library exports."""
    if path is None:
        return sorted(set(header_symbols(HEADER_PATH)) | set(header_symbols(DEBUG_HEADER_PATH)))
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)  # declarations only: the docs name other calls
    return sorted(set(re.findall(r"\b(mgicp_[a-z_0-9]+)\s*\(", text)))


def _mapped_hip_runtimes() -> set[str]:
    """Real paths of every HIP runtime (libamdhip64*) mapped into this process."""
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split(None, 5)
                if len(parts) == 6 and "libamdhip64" in os.path.basename(parts[5].strip()):
                    out.add(os.path.realpath(parts[5].strip()))
    except OSError:  # no procfs: nothing to check against
        pass
    return out


def _rocm_lib_dir() -> str:
    return os.path.realpath(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib"))


def check_single_hip_runtime(when: str) -> None:
    """libmgicp.so links ROCm's HIP runtime (/opt/rocm/lib/libamdhip64.so.7).  A second HIP runtime
    in the same process -- torch bundles its own (torch/lib/libamdhip64.so, a different ROCm
    release) and maps it at `import torch` -- was observed to corrupt the heap on MI355X ("double
    free or corruption" at teardown, round 1, parallel.py).  Refuse that combination loudly."""
    libs = _mapped_hip_runtimes()
    foreign = sorted(p for p in libs if os.path.dirname(p) != _rocm_lib_dir())
    if foreign or len(libs) > 1:
        raise MgicpError(
            MGICP_E_HIP,
            f"{when}: another HIP runtime is mapped in this process ({', '.join(sorted(libs))}); libmgicp.so "
            f"uses {_rocm_lib_dir()}/libamdhip64.so and two HIP runtimes in one process corrupt the heap. "
            "Do not import torch (or anything bundling its own HIP runtime) in a process that uses libmgicp.so.")


def load() -> ctypes.CDLL:
    """Load the in-tree libmgicp.so; raise loudly when it is absent (no fallback path) or when a
    second HIP runtime is (or would become) mapped next to it."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()' "
            "or `make`). There is no CPU fallback.")
    check_single_hip_runtime("before loading libmgicp.so")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    check_single_hip_runtime("after loading libmgicp.so")
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def default_params() -> MgicpParams:
    p = MgicpParams()
    load().mgicp_default_params(ctypes.byref(p))
    return p
