"""InitialAlignment -- the pre-alignment's steps that run on the MI355X engine.

Seven members of the reference class (src/InitialAlignment.cpp): obtainBoundaryKeypoints, the keypoint step
of the BOUNDARY (default) and NORMALS methods, obtainHarrisKeypoints, the keypoint step of HARRIS,
obtainFeatures, the FPFH descriptors at the keypoints (BOUNDARY and HARRIS), obtainCorrespondences, the
nearest target descriptor of every source descriptor, and the three steps that turn the correspondences
into rigid_tf_: rejectCorrespondences (RANSAC), rejectOneToOneCorrespondences and estimateTransform (SVD).
runKeypointsBasedAlgorithm chains them as the reference does, so BOUNDARY and HARRIS run on the engine from
the normals to the transform.  The normals they take come from gicp_alignment.getNormals (Utils::getNormals).

Of the NORMALS method: obtainNormalsCluster (normal-conditioned Euclidean clustering) and obtainDominantNormals,
chained by runNormalsBasedAlgorithm after the boundary keypoints as the reference does.  Out of scope:
getTransformationFromNormals and its helpers (normalsCorrespondences, findIdx, matrixFromAngles) -- O(clusters^2)
host arithmetic of the reference's own on at most 40 normals, which stays in the catkin package.
"""
from __future__ import annotations

import numpy as np

from .cloud import PointCloudRGB
from .engine import GICPEngine

BOUNDARY_K_SEARCH = 30             # detector.setKSearch(30)
BOUNDARY_ANGLE_THRESHOLD = 1.047   # detector.setAngleThreshold(1.047f)
RADIUS_FACTOR = 1.4                # radius_factor_ (the constructor's default)
HARRIS_THRESHOLD = np.float32(1e-6)  # detector.setThreshold(1e-6): PCL's threshold_ is a float
RANSAC_INLIER_THRESHOLD = 1.5      # rejector.setInlierThreshold(1.5)
RANSAC_MAX_ITERATIONS = 1000       # CorrespondenceRejectorSampleConsensus's default max_iterations_
NORMALS_CLUSTER_TOLERANCE = float(np.float32(0.05))  # const float tolerance = 0.05f
NORMALS_CLUSTER_EPS_ANGLE = 20 * (np.pi / 180.0)     # const double eps_angle = 20 * (M_PI / 180.0)
NORMALS_CLUSTER_PERCENTAJE = 0.025                   # min_cluster_size = (int)normals->size() * PERCENTAJE


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


def _xyz(cloud):
    return cloud.xyz() if isinstance(cloud, PointCloudRGB) else np.asarray(cloud, np.float32).reshape(-1, 3)


def rejectCorrespondences(source_keypoints, target_keypoints, correspondences, engine: GICPEngine | None = None):
    """InitialAlignment::rejectCorrespondences (src/InitialAlignment.cpp:519-530):
    pcl::registration::CorrespondenceRejectorSampleConsensus with an inlier threshold of 1.5, refinement and the
    rejector's 1000 iterations.  `correspondences` is obtainCorrespondences' triple; returns the remaining
    triple, in input order (all of it when PCL finds no model or the refinement fails)."""
    if engine is None:
        from .filter import _engine

        engine = _engine()
    iq, im, dist = (np.asarray(a) for a in correspondences)
    if len(iq) == 0:  # getCorrespondences leaves an empty input alone
        return iq, im, dist
    keep, _T, _info = engine.reject_ransac(source_keypoints, target_keypoints, iq, im, RANSAC_INLIER_THRESHOLD,
                                           RANSAC_MAX_ITERATIONS, True)
    return iq[keep], im[keep], dist[keep]


def rejectOneToOneCorrespondences(correspondences, n_target: int, engine: GICPEngine | None = None):
    """InitialAlignment::rejectOneToOneCorrespondences (src/InitialAlignment.cpp:532-538):
    pcl::registration::CorrespondenceRejectorOneToOne.  n_target bounds index_match (the target keypoints'
    number).  Returns the surviving triple in ascending index_match."""
    if engine is None:
        from .filter import _engine

        engine = _engine()
    iq, im, dist = (np.asarray(a) for a in correspondences)
    if len(iq) == 0:
        return iq, im, dist
    order, _info = engine.reject_one_to_one(im, dist, n_target)
    return iq[order], im[order], dist[order]


def estimateTransform(source_keypoints, target_keypoints, correspondences, engine: GICPEngine | None = None):
    """InitialAlignment::estimateTransform (src/InitialAlignment.cpp:540-545):
    pcl::registration::TransformationEstimationSVD over the correspondences.  Returns (rigid_tf float32[4, 4],
    transform_exists): the reference sets transform_exists_ when rigid_tf_ is not the zero matrix."""
    if engine is None:
        from .filter import _engine

        engine = _engine()
    iq, im, _dist = correspondences
    T, _info = engine.estimate_rigid_svd(source_keypoints, target_keypoints, iq, im)
    return T, bool(np.any(T != 0))


def runKeypointsBasedAlgorithm(source, target, method: str = "BOUNDARY", radius_factor: float = RADIUS_FACTOR,
                               engine: GICPEngine | None = None):
    """InitialAlignment::runKeypointsBasedAlgorithm (src/InitialAlignment.cpp:117-128) for the BOUNDARY and
    HARRIS methods: keypoints and features of both clouds, obtainCorrespondences, rejectCorrespondences,
    rejectOneToOneCorrespondences when more than source_cloud.size() / 2 (integer division) correspondences
    remain, estimateTransform.  `source` and `target` are (cloud, normals) pairs (normals: getNormals' array).
    Returns (rigid_tf float32[4, 4], transform_exists, steps): steps holds every intermediate result."""
    if method not in ("BOUNDARY", "HARRIS"):
        raise ValueError(f"method must be BOUNDARY or HARRIS, got {method!r}")
    if engine is None:
        from .filter import _engine

        engine = _engine()
    steps = {}
    for name, (cloud, normals) in (("source", source), ("target", target)):
        if method == "BOUNDARY":
            _status, kp, _non = obtainBoundaryKeypoints(cloud, normals, engine)
        else:
            _status, kp = obtainHarrisKeypoints(cloud, normals, radius_factor, engine)
        _status, features = obtainFeatures(cloud, normals, kp, radius_factor, engine)
        steps[name + "_keypoints_indices"] = kp
        steps[name + "_keypoints"] = np.ascontiguousarray(_xyz(cloud)[kp], np.float32)
        steps[name + "_features"] = features
    sk, tk = steps["source_keypoints"], steps["target_keypoints"]
    corr = obtainCorrespondences(steps["source_features"], steps["target_features"], engine)
    steps["correspondences"] = corr
    corr = rejectCorrespondences(sk, tk, corr, engine)
    steps["correspondences_ransac"] = corr
    source_size = source[0].size() if isinstance(source[0], PointCloudRGB) else len(_xyz(source[0]))
    steps["one_to_one"] = len(corr[0]) > source_size // 2
    if steps["one_to_one"]:
        corr = rejectOneToOneCorrespondences(corr, len(tk), engine)
    steps["correspondences_final"] = corr
    T, exists = estimateTransform(sk, tk, corr, engine)
    return T, exists, steps


def obtainNormalsCluster(cloud, normals, engine: GICPEngine | None = None):
    """InitialAlignment::obtainNormalsCluster (src/InitialAlignment.cpp:130-161): pcl::extractEuclideanClusters
    with normals at a tolerance of 0.05f, 20 degrees, a minimum size of (int)n * 0.025 truncated to unsigned
    and no cap.  Returns the clusters, int32 index arrays in ascending seed; when none is found, the
    reference's fallback of one cluster 0 .. n - 1."""
    if engine is None:
        from .filter import _engine

        engine = _engine()
    normals = np.asarray(normals, dtype=np.float32)
    n = len(normals)
    min_size = int(int(n) * NORMALS_CLUSTER_PERCENTAJE)
    clusters, _labels, _info = engine.normal_clusters(cloud, normals, NORMALS_CLUSTER_TOLERANCE,
                                                      NORMALS_CLUSTER_EPS_ANGLE, min_size, 0)
    if len(clusters) == 0:
        size = cloud.size() if isinstance(cloud, PointCloudRGB) else len(np.asarray(cloud).reshape(-1, 3))
        clusters = [np.arange(size, dtype=np.int32)]
    return clusters


def obtainDominantNormals(normals, clusters, engine: GICPEngine | None = None):
    """InitialAlignment::obtainDominantNormals (src/InitialAlignment.cpp:163-187): float32 [len(clusters), 3],
    per cluster the normalised sum of its normals, the first member counted twice as the reference does."""
    if engine is None:
        from .filter import _engine

        engine = _engine()
    return engine.dominant_normals(normals, clusters)


def runNormalsBasedAlgorithm(source, target, engine: GICPEngine | None = None):
    """InitialAlignment::runNormalsBasedAlgorithm (src/InitialAlignment.cpp:81-115) up to the dominant normals:
    boundary keypoints of both clouds, the extraction of the non-boundary records (cloud and normals),
    obtainNormalsCluster and obtainDominantNormals.  `source` and `target` are (cloud, normals) pairs.  Returns
    (source_dominant_normals, target_dominant_normals, steps); getTransformationFromNormals is out of scope
    (module docstring)."""
    if engine is None:
        from .filter import _engine

        engine = _engine()
    steps, dominant = {}, []
    for name, (cloud, normals) in (("source", source), ("target", target)):
        normals = np.asarray(normals, dtype=np.float32)
        _status, _kp, non_boundary = obtainBoundaryKeypoints(cloud, normals, engine)
        xyz = np.ascontiguousarray(_xyz(cloud)[non_boundary], np.float32)
        nrm = np.ascontiguousarray(normals[non_boundary], np.float32)
        clusters = obtainNormalsCluster(xyz, nrm, engine)
        dominant.append(obtainDominantNormals(nrm, clusters, engine))
        steps[name + "_non_boundary_indices"] = non_boundary
        steps[name + "_cloud_no_boundary"] = xyz
        steps[name + "_normals_no_boundary"] = nrm
        steps[name + "_cluster_indices"] = clusters
    return dominant[0], dominant[1], steps
