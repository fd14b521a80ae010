/*
 * adapter/InitialAlignment_features_mi355x.cpp -- InitialAlignment::obtainFeatures over the MI355X engine.
 * Replaces the body of
 *     InitialAlignment::obtainFeatures   (src/InitialAlignment.cpp:487-508 of the reference:
 *                          pcl::FPFHEstimation<PointXYZRGB, Normal, FPFHSignature33> at the keypoint
 *                          indices, radius search of radius_factor_ * cloud resolution over a fresh
 *                          kd-tree; the BOUNDARY and HARRIS methods call it on both clouds)
 * Delete that definition from src/InitialAlignment.cpp and add this file to the library sources
 * (INTEGRATION.md section 2); the other members keep their reference implementations.
 * Compiled inside the catkin workspace.
 */
#include <InitialAlignment.h>

#include <mi355x_gicp.h>

#include <cstddef>
#include <mutex>

namespace
{
static_assert(sizeof(pcl::PointXYZRGB) == 32, "PointXYZRGB record must be 32 bytes (x,y,z,pad,rgb,pad)");
static_assert(sizeof(pcl::Normal) == 32, "pcl::Normal record must be 32 bytes (normal[3], pad, curvature, pad)");
static_assert(sizeof(pcl::FPFHSignature33) == 132, "FPFHSignature33 record must be 33 floats");

// one engine context per process for this member; a context serves one caller at a time
// (include/mi355x_gicp.h "Threading"), so every use takes the mutex
std::mutex& featuresMutex()
{
    static std::mutex m;
    return m;
}

mgicp_ctx* featuresContext()
{
    static mgicp_ctx* ctx = []() {
        mgicp_ctx* c = nullptr;
        if (mgicp_create(&c, nullptr) != MGICP_OK)
        {
            ROS_ERROR("MI355X engine unavailable: no HIP device?");
            return static_cast<mgicp_ctx*>(nullptr);
        }
        return c;
    }();
    return ctx;
}
}  // namespace

int InitialAlignment::obtainFeatures(PointCloudRGB::Ptr cloud,
                                     PointCloudNormal::Ptr normals,
                                     pcl::IndicesPtr keypoints_indices,
                                     PointCloudFPFH::Ptr features)
{
    const size_t n = cloud->points.size();
    const size_t nk = keypoints_indices->size();
    // Feature::compute empties the output first; normals that do not match the cloud fail its initCompute
    features->points.clear();
    features->width = features->height = 0;
    if (normals->points.size() != n || n == 0 || nk == 0)
        return -1;

    std::lock_guard<std::mutex> lock(featuresMutex());
    mgicp_ctx* ctx = featuresContext();
    if (!ctx)
        return -1;
    double cloud_res = 0.0;
    int rc = mgicp_cloud_resolution(ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB), &cloud_res);
    if (rc != MGICP_OK)
    {
        ROS_ERROR("cloud resolution failed (%d): %s", rc, mgicp_last_error(ctx));
        return -1;
    }
    double feature_radius = cloud_res * radius_factor_;

    features->points.resize(nk);
    mgicp_fpfh_info info;
    rc = mgicp_fpfh_features(ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB), &normals->points[0].normal_x,
                             sizeof(pcl::Normal), keypoints_indices->data(), nk, feature_radius,
                             features->points[0].histogram, sizeof(pcl::FPFHSignature33), nullptr, nullptr, &info);
    if (rc != MGICP_OK)
    {
        ROS_ERROR("FPFH estimation failed (%d): %s", rc, mgicp_last_error(ctx));
        features->points.clear();
        return -1;
    }
    features->header = cloud->header;
    features->width = static_cast<std::uint32_t>(nk);
    features->height = 1;
    features->is_dense = info.n_nan == 0;

    if (features->size() == 0) return -1;

    return 0;
}
