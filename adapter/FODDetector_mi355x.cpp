/*
 * adapter/FODDetector_mi355x.cpp -- FODDetector::clusterPossibleFODs over the MI355X engine.
 * Replaces the body of
 *     FODDetector::clusterPossibleFODs   (src/FODDetector.cpp:45-58 of the reference,
 *                                         pcl::EuclideanClusterExtraction over a kd-tree)
 * Delete that definition from src/FODDetector.cpp and add this file to the library sources
 * (INTEGRATION.md section 2); the constructor, the setters and the fodIndicesTo* members keep their
 * reference implementations.  Compiled inside the catkin workspace.
 */
#include <FODDetector.h>

#include <EngineContext_mi355x.h>
#include <mi355x_gicp.h>

#include <cstddef>
#include <vector>

namespace
{
static_assert(sizeof(pcl::PointXYZRGB) == 32, "PointXYZRGB record must be 32 bytes (x,y,z,pad,rgb,pad)");
}  // namespace

void FODDetector::clusterPossibleFODs()
{
    cluster_indices_.clear();
    const size_t n = cloud_ ? cloud_->points.size() : 0;
    std::lock_guard<std::mutex> lock(mi355x::helperMutex());
    mgicp_ctx* ctx = mi355x::helperContext();
    if (!ctx)
        return;
    // EuclideanClusterExtraction::setMinClusterSize(int): the double is truncated.  The conversion is
    // defined only inside int's range: NaN and values below 1 ask for every cluster (size >= 1), values
    // past INT_MAX stay there (no cluster can be that large)
    int min_pts = 0;
    if (min_cluster_size_ >= 2147483647.0)
        min_pts = 2147483647;
    else if (min_cluster_size_ >= 1.0)
        min_pts = static_cast<int>(min_cluster_size_);
    std::vector<int> labels(n), indices(n);
    std::vector<size_t> offsets(n + 1, 0);
    mgicp_cluster_info info;
    const int rc = mgicp_euclidean_clusters(ctx, n ? &cloud_->points[0].x : nullptr, n, sizeof(pcl::PointXYZRGB),
                                            cluster_tolerance_, min_pts > 0 ? static_cast<size_t>(min_pts) : 0, 0,
                                            labels.data(), indices.data(), offsets.data(), &info);
    if (rc != MGICP_OK)
    {
        ROS_ERROR("euclidean clustering failed (%d): %s", rc, mgicp_last_error(ctx));
        return;
    }
    cluster_indices_.resize(static_cast<size_t>(info.n_clusters));
    for (size_t c = 0; c < cluster_indices_.size(); ++c)
    {
        cluster_indices_[c].header = cloud_->header;
        cluster_indices_[c].indices.assign(indices.begin() + static_cast<std::ptrdiff_t>(offsets[c]),
                                           indices.begin() + static_cast<std::ptrdiff_t>(offsets[c + 1]));
    }
    ROS_INFO("cluster_indices_size: %zd", cluster_indices_.size());
}
