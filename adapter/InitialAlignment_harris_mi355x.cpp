/*
 * adapter/InitialAlignment_harris_mi355x.cpp -- InitialAlignment::obtainHarrisKeypoints over the MI355X engine.
 * Replaces the body of
 *     InitialAlignment::obtainHarrisKeypoints   (src/InitialAlignment.cpp:399-424 of the reference:
 *                          pcl::HarrisKeypoint3D with setNonMaxSupression(true), setThreshold(1e-6) and
 *                          setRadius(radius_factor_ * resolution); the HARRIS method calls it on both clouds)
 * Delete that definition from src/InitialAlignment.cpp and add this file to the library sources
 * (INTEGRATION.md section 2); the other members keep their reference implementations.
 * Compiled inside the catkin workspace.
 */
#include <Filter.h>
#include <InitialAlignment.h>

#include <mi355x_gicp.h>

#include <cstddef>
#include <mutex>
#include <vector>

namespace
{
static_assert(sizeof(pcl::PointXYZRGB) == 32, "PointXYZRGB record must be 32 bytes (x,y,z,pad,rgb,pad)");
static_assert(sizeof(pcl::Normal) == 32, "pcl::Normal record must be 32 bytes (normal[3], pad, curvature, pad)");

// one engine context per process for this member; a context serves one caller at a time
// (include/mi355x_gicp.h "Threading"), so every use takes the mutex
std::mutex& harrisMutex()
{
    static std::mutex m;
    return m;
}

mgicp_ctx* harrisContext()
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

int InitialAlignment::obtainHarrisKeypoints(PointCloudRGB::Ptr cloud,
                                            PointCloudNormal::Ptr normals,
                                            PointCloudRGB::Ptr keypoints_cloud,
                                            pcl::IndicesPtr keypoints_indices)
{
    const size_t n = cloud->points.size();
    // Keypoint::initCompute refuses normals that do not match the cloud: no keypoint, the reference's -1
    if (normals->points.size() != n || n == 0)
        return -1;

    std::vector<int> found(n);
    size_t n_found = 0;
    {
        std::lock_guard<std::mutex> lock(harrisMutex());
        mgicp_ctx* ctx = harrisContext();
        if (!ctx)
            return -1;
        double cloud_res = 0.0;
        int rc = mgicp_cloud_resolution(ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB), &cloud_res);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("cloud resolution failed (%d): %s", rc, mgicp_last_error(ctx));
            return -1;
        }
        double keypoint_radius = cloud_res * radius_factor_;
        // setRadius and setThreshold take floats
        rc = mgicp_harris_keypoints(ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB),
                                    &normals->points[0].normal_x, sizeof(pcl::Normal),
                                    static_cast<float>(keypoint_radius), static_cast<float>(1e-6), 1, found.data(),
                                    &n_found, nullptr, nullptr, nullptr, nullptr);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("Harris keypoints failed (%d): %s", rc, mgicp_last_error(ctx));
            return -1;
        }
    }

    if (n_found == 0) return -1;

    keypoints_indices->assign(found.begin(), found.begin() + static_cast<std::ptrdiff_t>(n_found));
    Filter::extractIndices(cloud, keypoints_cloud, keypoints_indices);

    return 0;
}
