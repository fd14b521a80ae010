"""InitialAlignment -- the pre-alignment's steps that run on the MI355X engine.

Four members of the reference class (src/InitialAlignment.cpp): obtainBoundaryKeypoints, the keypoint step
of the BOUNDARY (default) and NORMALS methods, obtainHarrisKeypoints, the keypoint step of HARRIS,
obtainFeatures, the FPFH descriptors at the keypoints (BOUNDARY and HARRIS), and obtainCorrespondences, the
nearest target descriptor of every source descriptor.  BOUNDARY and HARRIS thus run on the engine from the
normals to the correspondences.  The normals they take come from gicp_alignment.getNormals
(Utils::getNormals).  Only the rejectors (rejectCorrespondences, rejectOneToOneCorrespondences) and
estimateTransform remain off the engine.
"""
from __future__ import annotations

import numpy as np

from .cloud import PointCloudRGB
from .engine import GICPEngine

BOUNDARY_K_SEARCH = 30             # detector.setKSearch(30)
BOUNDARY_ANGLE_THRESHOLD = 1.047   # detector.setAngleThreshold(1.047f)
RADIUS_FACTOR = 1.4                # radius_factor_ (the constructor's default)
HARRIS_THRESHOLD = np.float32(1e-6)  # detector.setThreshold(1e-6): PCL's threshold_ is a float


def obtainBoundaryKeypoints(cloud, normals, engine: GICPEngine | None = None):
    """InitialAlignment::obtainBoundaryKeypoints (src/InitialAlignment.cpp:426-456):
    pcl::BoundaryEstimation with a 30-search and an angle threshold of 1.047 rad.  `normals` is float32
    [n, 3] or [n, 4] (getNormals' array).  Returns (status, keypoints_indices, non_keypoints_indices), the
    indices ascending int32 arrays: status -1 when len(normals) != len(cloud) (PCL's initCompute fails, the
    output stays empty and its size differs from the cloud's; both index arrays are empty) or when no
    keypoint is found, else 0.  The keypoint cloud is cloud[keypoints_indices]."""
    size = cloud.size() if isinstance(cloud, PointCloudRGB) else len(np.asarray(cloud).reshape(-1, 3))
    normals = np.asarray(normals, dtype=np.float32)
    empty = np.zeros(0, np.int32)
    if normals.ndim != 2 or len(normals) != size:
        return -1, empty, empty
    if engine is None:
        from .filter import _engine

        engine = _engine()
    boundary, _gap, _nn, _info = engine.boundary_points(cloud, normals, BOUNDARY_K_SEARCH, BOUNDARY_ANGLE_THRESHOLD)
    keypoints = np.flatnonzero(boundary).astype(np.int32)
    non_keypoints = np.flatnonzero(~boundary).astype(np.int32)
    return (-1 if len(keypoints) == 0 else 0), keypoints, non_keypoints


def obtainHarrisKeypoints(cloud, normals, radius_factor: float = RADIUS_FACTOR, engine: GICPEngine | None = None):
    """InitialAlignment::obtainHarrisKeypoints (src/InitialAlignment.cpp:399-424): pcl::HarrisKeypoint3D with
    non-maximum suppression, a threshold of float32(1e-6) and a radius of
    float32(computeCloudResolution(cloud) * radius_factor) (PCL's setRadius takes a float).  `normals` is
    float32 [n, 3] or [n, 4] (getNormals' array).  Returns (status, keypoints_indices), the indices an
    ascending int32 array: status -1 when len(normals) != len(cloud) or when no keypoint is found, else 0.
    The keypoint cloud is cloud[keypoints_indices]."""
    size = cloud.size() if isinstance(cloud, PointCloudRGB) else len(np.asarray(cloud).reshape(-1, 3))
    normals = np.asarray(normals, dtype=np.float32)
    if normals.ndim != 2 or len(normals) != size:
        return -1, np.zeros(0, np.int32)
    if engine is None:
        from .filter import _engine

        engine = _engine()
    radius = float(np.float32(engine.cloud_resolution(cloud) * radius_factor))
    keypoints, _resp, _cov, _cnt, _info = engine.harris_keypoints(cloud, normals, radius, HARRIS_THRESHOLD, True)
    return (-1 if len(keypoints) == 0 else 0), keypoints


def obtainFeatures(cloud, normals, keypoints_indices, radius_factor: float = RADIUS_FACTOR,
                   engine: GICPEngine | None = None):
    """InitialAlignment::obtainFeatures (src/InitialAlignment.cpp:487-508): pcl::FPFHEstimation at
    `keypoints_indices` with a radius search of radius_factor * computeCloudResolution(cloud).  `normals` is
    float32 [n, 3] or [n, 4] (getNormals' array).  Returns (status, features): features float32
    [len(keypoints_indices), 33], one FPFHSignature33 per keypoint in the order given; status -1 when no
    feature comes back (no keypoint, or normals that do not match the cloud: PCL's initCompute fails and
    the output stays empty), else 0."""
    size = cloud.size() if isinstance(cloud, PointCloudRGB) else len(np.asarray(cloud).reshape(-1, 3))
    normals = np.asarray(normals, dtype=np.float32)
    keypoints = np.asarray(keypoints_indices, dtype=np.int32).reshape(-1)
    empty = np.zeros((0, 33), np.float32)
    if normals.ndim != 2 or len(normals) != size or len(keypoints) == 0:
        return -1, empty
    if engine is None:
        from .filter import _engine

        engine = _engine()
    radius = engine.cloud_resolution(cloud) * radius_factor
    features, _counts, _sizes, _info = engine.fpfh_features(cloud, normals, keypoints, radius)
    return (-1 if len(features) == 0 else 0), features


def obtainCorrespondences(source_features, target_features, engine: GICPEngine | None = None):
    """InitialAlignment::obtainCorrespondences (src/InitialAlignment.cpp:510-517):
    pcl::registration::CorrespondenceEstimation::determineCorrespondences with its default max_distance
    (nothing rejected).  The features are float32 [n, 33] (obtainFeatures' arrays).  Returns (index_query
    int32[m], index_match int32[m], distance float32[m]) -- the fields of pcl::Correspondences, one entry per
    source feature that found a target, in ascending index_query; distance is the squared L2 distance."""
    if engine is None:
        from .filter import _engine

        engine = _engine()
    match, distance, _info = engine.match_features(source_features, target_features)
    index_query = np.flatnonzero(match >= 0).astype(np.int32)
    return index_query, match[index_query], distance[index_query]
