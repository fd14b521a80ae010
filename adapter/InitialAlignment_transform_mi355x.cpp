/*
 * adapter/InitialAlignment_transform_mi355x.cpp -- the three members of InitialAlignment that turn the
 * correspondences into rigid_tf_, over the MI355X engine.  Replaces the bodies of (src/InitialAlignment.cpp
 * of the reference)
 *     InitialAlignment::rejectCorrespondences          (:519-530: pcl::registration::
 *                          CorrespondenceRejectorSampleConsensus<PointXYZRGB> from source_keypoints_ to
 *                          target_keypoints_ with setInlierThreshold(1.5), setRefineModel(true) and the
 *                          rejector's default of 1000 iterations, correspondences_ as input and output)
 *     InitialAlignment::rejectOneToOneCorrespondences  (:532-538: pcl::registration::
 *                          CorrespondenceRejectorOneToOne on correspondences_, in place)
 *     InitialAlignment::estimateTransform              (:540-545: pcl::registration::
 *                          TransformationEstimationSVD<PointXYZRGB, PointXYZRGB> over correspondences_ into
 *                          rigid_tf_; transform_exists_ is set when rigid_tf_ is not the zero matrix)
 * Delete those three definitions from src/InitialAlignment.cpp and add this file to the library sources
 * beside adapter/InitialAlignment_mi355x.cpp; runKeypointsBasedAlgorithm itself
 * stays the reference's.  Compiled inside the catkin workspace.
 */
#include <InitialAlignment.h>

#include <EngineContext_mi355x.h>
#include <mi355x_gicp.h>

#include <cstddef>
#include <vector>

namespace
{
static_assert(sizeof(pcl::PointXYZRGB) == 32, "PointXYZRGB record must be 32 bytes (x,y,z,pad,rgb,pad)");

// the three fields of the correspondences as the parallel arrays the engine takes
void split(const pcl::Correspondences& corr, std::vector<int>& query, std::vector<int>& match,
           std::vector<float>& distance)
{
    query.resize(corr.size());
    match.resize(corr.size());
    distance.resize(corr.size());
    for (size_t i = 0; i < corr.size(); ++i)
    {
        query[i] = corr[i].index_query;
        match[i] = corr[i].index_match;
        distance[i] = corr[i].distance;
    }
}

const float* xyzOf(const pcl::PointCloud<pcl::PointXYZRGB>& cloud)
{
    return cloud.points.empty() ? nullptr : &cloud.points[0].x;
}
}  // namespace

void InitialAlignment::rejectCorrespondences()
{
    const size_t m = correspondences_->size();
    // getCorrespondences leaves an empty input alone
    if (m != 0)
    {
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
        if (!ctx)
            return;
        std::vector<int> query, match;
        std::vector<float> distance;
        split(*correspondences_, query, match, distance);
        std::vector<unsigned char> keep(m);
        size_t n_keep = 0;
        float best_transformation[16];
        const int rc = mgicp_reject_ransac(ctx, xyzOf(*source_keypoints_), source_keypoints_->points.size(),
                                           sizeof(pcl::PointXYZRGB), xyzOf(*target_keypoints_),
                                           target_keypoints_->points.size(), sizeof(pcl::PointXYZRGB), query.data(),
                                           match.data(), m, 1.5, 1000, 1, keep.data(), &n_keep, best_transformation,
                                           nullptr);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("correspondence rejection failed (%d): %s", rc, mgicp_last_error(ctx));
            return;
        }
        // the remaining correspondences, in input order.  pcl::Correspondence has a virtual destructor:
        // moved field by field
        size_t k = 0;
        for (size_t i = 0; i < m; ++i)
        {
            if (!keep[i])
                continue;
            pcl::Correspondence& c = (*correspondences_)[k++];
            c.index_query = query[i];
            c.index_match = match[i];
            c.distance = distance[i];
        }
        correspondences_->resize(k);
    }
    ROS_INFO("th: %f", 1.5);
    ROS_INFO("Filtered %zd correspondences", correspondences_->size());
}

void InitialAlignment::rejectOneToOneCorrespondences()
{
    const size_t m = correspondences_->size();
    if (m != 0)
    {
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
        if (!ctx)
            return;
        std::vector<int> query, match;
        std::vector<float> distance;
        split(*correspondences_, query, match, distance);
        // the rejector knows no target cloud: the largest index bounds it
        size_t n_target = 0;
        for (size_t i = 0; i < m; ++i)
            if (match[i] >= 0 && static_cast<size_t>(match[i]) >= n_target)
                n_target = static_cast<size_t>(match[i]) + 1;
        std::vector<int> order(m);
        size_t n_keep = 0;
        const int rc = mgicp_reject_one_to_one(ctx, match.data(), distance.data(), m, n_target, order.data(), &n_keep,
                                               nullptr);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("one-to-one rejection failed (%d): %s", rc, mgicp_last_error(ctx));
            return;
        }
        for (size_t k = 0; k < n_keep; ++k)
        {
            pcl::Correspondence& c = (*correspondences_)[k];
            const size_t i = static_cast<size_t>(order[k]);
            c.index_query = query[i];
            c.index_match = match[i];
            c.distance = distance[i];
        }
        correspondences_->resize(n_keep);
    }
    ROS_INFO("Found %zd one to one correspondences:", correspondences_->size());
}

void InitialAlignment::estimateTransform()
{
    {
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
        if (!ctx)
            return;
        std::vector<int> query, match;
        std::vector<float> distance;
        split(*correspondences_, query, match, distance);
        float transform[16];
        const int rc = mgicp_estimate_rigid_svd(ctx, xyzOf(*source_keypoints_), source_keypoints_->points.size(),
                                                sizeof(pcl::PointXYZRGB), xyzOf(*target_keypoints_),
                                                target_keypoints_->points.size(), sizeof(pcl::PointXYZRGB),
                                                query.data(), match.data(), query.size(), transform, nullptr);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("transform estimation failed (%d): %s", rc, mgicp_last_error(ctx));
            return;
        }
        // Eigen::Matrix4f is column-major, as the engine's transforms are
        for (int i = 0; i < 16; ++i)
            rigid_tf_.data()[i] = transform[i];
    }
    // the reference's rigid_tf_ != Eigen::Matrix4f::Zero()
    for (int i = 0; i < 16; ++i)
        if (rigid_tf_.data()[i] != 0.f)
            transform_exists_ = true;
}
