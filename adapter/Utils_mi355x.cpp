/*
 * adapter/Utils_mi355x.cpp -- Utils::getNormals over the MI355X engine.
 * Replaces the body of
 *     Utils::getNormals   (src/Utils.cpp:27-44 of the reference, pcl::NormalEstimation with a radius
 *                          search over a kd-tree; InitialAlignment.cpp:69-70 and
 *                          GICPAlignment::getCovariances call it)
 * Delete that definition from src/Utils.cpp and add this file to the library sources
 * (INTEGRATION.md section 2); the other Utils members keep their reference implementations.
 * Compiled inside the catkin workspace.
 */
#include <Utils.h>

#include <EngineContext_mi355x.h>
#include <mi355x_gicp.h>

#include <cstddef>
#include <vector>

namespace
{
static_assert(sizeof(pcl::PointXYZRGB) == 32, "PointXYZRGB record must be 32 bytes (x,y,z,pad,rgb,pad)");
static_assert(sizeof(pcl::Normal) == 32, "pcl::Normal record must be 32 bytes (normal[3], pad, curvature, pad)");
static_assert(offsetof(pcl::Normal, curvature) == 16, "pcl::Normal::curvature sits at byte 16");
}  // namespace

bool Utils::getNormals(PointCloudRGB::Ptr& cloud, double normal_radius, PointCloudNormal::Ptr& normals)
{
    ROS_INFO("Computing normals with radius: %f", normal_radius);
    const size_t n = cloud ? cloud->points.size() : 0;
    // Feature::compute: the output takes the input's header and, on failure, is left empty
    normals->header = cloud ? cloud->header : pcl::PCLHeader();
    normals->points.clear();
    normals->width = normals->height = 0;
    std::lock_guard<std::mutex> lock(mi355x::helperMutex());
    mgicp_ctx* ctx = mi355x::helperContext();
    if (ctx)
    {
        std::vector<pcl::Normal> out(n);  // data_n[3] = 0 and the pads from the constructor
        std::vector<float> curvature(n);
        mgicp_normals_info info;
        const int rc = mgicp_estimate_normals(ctx, n ? &cloud->points[0].x : nullptr, n, sizeof(pcl::PointXYZRGB),
                                              normal_radius, nullptr, n ? &out[0].normal_x : nullptr, sizeof(pcl::Normal),
                                              n ? curvature.data() : nullptr, nullptr, &info);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("normal estimation failed (%d): %s", rc, mgicp_last_error(ctx));
        }
        else
        {
            for (size_t i = 0; i < n; ++i)
                out[i].curvature = curvature[i];
            normals->points.swap(out);
            // Feature::compute keeps the input's organisation; computeFeature clears is_dense at the first NaN
            normals->width = cloud ? cloud->width : 0;
            normals->height = cloud ? cloud->height : 0;
            if (static_cast<size_t>(normals->width) * normals->height != n)
            {
                normals->width = static_cast<std::uint32_t>(n);
                normals->height = 1;
            }
            normals->is_dense = info.n_nan == 0;
        }
    }

    // the reference's return rule (src/Utils.cpp:41-43): one normal per input point
    return normals->points.size() == n;
}
