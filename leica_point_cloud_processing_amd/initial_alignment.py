"""InitialAlignment -- the pre-alignment's steps that run on the MI355X engine.

So far one member of the reference class (src/InitialAlignment.cpp): obtainBoundaryKeypoints, the keypoint
step of the BOUNDARY (default) and NORMALS methods.  The normals it takes come from
gicp_alignment.getNormals (Utils::getNormals); FPFH at the keypoints, the feature correspondences and the
RANSAC rejector are not on the engine yet.
"""
from __future__ import annotations

import numpy as np

from .cloud import PointCloudRGB
from .engine import GICPEngine

BOUNDARY_K_SEARCH = 30             # detector.setKSearch(30)
BOUNDARY_ANGLE_THRESHOLD = 1.047   # detector.setAngleThreshold(1.047f)


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
