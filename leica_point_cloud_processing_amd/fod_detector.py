"""FODDetector -- the reference's last inspection step: Euclidean clustering of the difference cloud.

Mirrors the reference class (include/FODDetector.h, src/FODDetector.cpp): FODDetectionState builds it
over the cloud Filter::removeFromCloud left, calls clusterPossibleFODs() (pcl::EuclideanClusterExtraction
over a kd-tree) and fodIndicesToPointCloud() for the count it publishes
(src/LeicaStateMachine.cpp:196-204).  The clustering runs on the GPU through libmgicp.so
(mgicp_euclidean_clusters); there is no CPU path.  The ROS-message variant (fodIndicesToROSMsg) is out
of scope here.
"""
from __future__ import annotations

import logging

import numpy as np

from .cloud import PointCloudRGB
from .filter import _engine

log = logging.getLogger(__name__)

DEFAULT_CLUSTER_TOLERANCE = 4e-3


class FODDetector:
    def __init__(self, cloud: PointCloudRGB, cluster_tolerance: float, min_fod_points: float):
        self.cloud_ = cloud
        self.cluster_indices_: list[np.ndarray] = []
        self.last_info: dict | None = None
        self.setClusterTolerance(cluster_tolerance)
        self.setMinFODpoints(min_fod_points)

    def setClusterTolerance(self, tolerance: float) -> None:
        if tolerance == 0:
            log.warning("FODDetector: invalid tolerance value: %f", tolerance)
            self.cluster_tolerance_ = DEFAULT_CLUSTER_TOLERANCE
        else:
            self.cluster_tolerance_ = float(tolerance)
        log.info("FODDetector: cluster tolerance set to: %f", self.cluster_tolerance_)

    def setMinFODpoints(self, min_fod_points: float) -> None:
        """Kept as the reference's double; EuclideanClusterExtraction::setMinClusterSize takes an int,
        so the value is truncated when it is used."""
        self.min_cluster_size_ = float(min_fod_points)

    def minClusterSize(self) -> int:
        """The int PCL's setter would hold: truncated; NaN and values below 1 ask for every cluster."""
        v = self.min_cluster_size_
        if not v >= 1.0:
            return 0
        return int(min(v, 2147483647.0))

    def clusterPossibleFODs(self) -> None:
        clusters, _labels, info = _engine().euclidean_clusters(
            self.cloud_, self.cluster_tolerance_, min_size=max(self.minClusterSize(), 0), max_size=0)
        self.cluster_indices_ = clusters
        self.last_info = info
        log.info("cluster_indices_size: %d", len(clusters))

    def getFODIndices(self) -> list[np.ndarray]:
        return [c.copy() for c in self.cluster_indices_]

    def fodIndicesToPointCloud(self) -> tuple[int, list[PointCloudRGB]]:
        """(number of possible FODs, one cloud per cluster holding copies of its records in index order)."""
        out = []
        for idx in self.cluster_indices_:
            c = PointCloudRGB()
            c.points = self.cloud_.points[idx].copy()
            log.info("cluster_size: %d", c.size())
            out.append(c)
        return len(out), out
