/*
 * adapter/InitialAlignment_mi355x.cpp -- InitialAlignment::obtainBoundaryKeypoints over the MI355X engine.
 * Replaces the body of
 *     InitialAlignment::obtainBoundaryKeypoints   (src/InitialAlignment.cpp:426-456 of the reference:
 *                          pcl::BoundaryEstimation with setKSearch(30) and setAngleThreshold(1.047f)
 *                          over a kd-tree; the BOUNDARY and NORMALS methods call it on both clouds)
 * Delete that definition from src/InitialAlignment.cpp and add this file to the library sources
 * (INTEGRATION.md section 2); the other members keep their reference implementations.
 * Compiled inside the catkin workspace.
 */
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
std::mutex& boundaryMutex()
{
    static std::mutex m;
    return m;
}

mgicp_ctx* boundaryContext()
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

int InitialAlignment::obtainBoundaryKeypoints(PointCloudRGB::Ptr cloud,
                                              PointCloudNormal::Ptr normals,
                                              PointCloudRGB::Ptr keypoints_cloud,
                                              pcl::IndicesPtr keypoints_indices,
                                              pcl::IndicesPtr non_keypoints_indices)
{
    const size_t n = cloud->points.size();
    // Feature::initCompute refuses normals that do not match the cloud: the output stays empty, and the
    // reference returns -1 when its size differs from the cloud's
    if (normals->points.size() != n)
        return -1;
    std::vector<unsigned char> boundary(n, 0);
    if (n > 0)
    {
        std::lock_guard<std::mutex> lock(boundaryMutex());
        mgicp_ctx* ctx = boundaryContext();
        if (!ctx)
            return -1;
        const int rc = mgicp_boundary_points(ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB),
                                             &normals->points[0].normal_x, sizeof(pcl::Normal), 30, 1.047f,
                                             boundary.data(), nullptr, nullptr, nullptr);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("boundary estimation failed (%d): %s", rc, mgicp_last_error(ctx));
            return -1;
        }
    }

    for (size_t i = 0; i < n; i++)
    {
        if (boundary[i] == 1)
        {
            keypoints_indices->push_back(static_cast<int>(i));
            keypoints_cloud->points.push_back(cloud->points[i]);
        }
        else
            non_keypoints_indices->push_back(static_cast<int>(i));
    }

    if (keypoints_indices->size() == 0)
        return -1;

    return 0;
}
