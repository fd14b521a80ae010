/*
 * adapter/InitialAlignment_mi355x.cpp -- the four keypoint-path members of InitialAlignment over the MI355X
 * engine.  Replaces the bodies of (src/InitialAlignment.cpp of the reference)
 *     InitialAlignment::obtainHarrisKeypoints     (:399-424: pcl::HarrisKeypoint3D with
 *                          setNonMaxSupression(true), setThreshold(1e-6) and setRadius(radius_factor_ *
 *                          resolution); the HARRIS method calls it on both clouds)
 *     InitialAlignment::obtainBoundaryKeypoints   (:426-456: pcl::BoundaryEstimation with setKSearch(30) and
 *                          setAngleThreshold(1.047f) over a kd-tree; the BOUNDARY and NORMALS methods call
 *                          it on both clouds)
 *     InitialAlignment::obtainFeatures            (:487-508: pcl::FPFHEstimation<PointXYZRGB, Normal,
 *                          FPFHSignature33> at the keypoint indices, radius search of radius_factor_ * cloud
 *                          resolution over a fresh kd-tree; the BOUNDARY and HARRIS methods call it on both
 *                          clouds)
 *     InitialAlignment::obtainCorrespondences     (:510-517: pcl::registration::CorrespondenceEstimation<
 *                          FPFHSignature33, FPFHSignature33>::determineCorrespondences from
 *                          source_features_ to target_features_, its max_distance left at the default;
 *                          every keypoint method calls it)
 * Delete those four definitions from src/InitialAlignment.cpp and add this file to the library sources
 * (INTEGRATION.md section 2); the other members keep their reference implementations.
 * Compiled inside the catkin workspace.
 */
#include <Filter.h>
#include <InitialAlignment.h>

#include <EngineContext_mi355x.h>
#include <mi355x_gicp.h>

#include <cfloat>
#include <cstddef>
#include <vector>

namespace
{
static_assert(sizeof(pcl::PointXYZRGB) == 32, "PointXYZRGB record must be 32 bytes (x,y,z,pad,rgb,pad)");
static_assert(sizeof(pcl::Normal) == 32, "pcl::Normal record must be 32 bytes (normal[3], pad, curvature, pad)");
static_assert(sizeof(pcl::FPFHSignature33) == 132, "FPFHSignature33 record must be 33 floats");

// the radius of the Harris keypoints and of the features: the cloud's resolution times radius_factor_.
// false: the resolution failed (logged).  The caller holds the helper mutex; the cloud is not empty
bool scaledResolution(mgicp_ctx* ctx, const pcl::PointCloud<pcl::PointXYZRGB>& cloud, double radius_factor,
                      double& radius)
{
    double cloud_res = 0.0;
    const int rc = mgicp_cloud_resolution(ctx, &cloud.points[0].x, cloud.points.size(), sizeof(pcl::PointXYZRGB),
                                          &cloud_res);
    if (rc != MGICP_OK)
    {
        ROS_ERROR("cloud resolution failed (%d): %s", rc, mgicp_last_error(ctx));
        return false;
    }
    radius = cloud_res * radius_factor;
    return true;
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
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
        if (!ctx)
            return -1;
        double keypoint_radius = 0.0;
        if (!scaledResolution(ctx, *cloud, radius_factor_, keypoint_radius))
            return -1;
        // setRadius and setThreshold take floats
        const int rc = mgicp_harris_keypoints(ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB),
                                              &normals->points[0].normal_x, sizeof(pcl::Normal),
                                              static_cast<float>(keypoint_radius), static_cast<float>(1e-6), 1,
                                              found.data(), &n_found, nullptr, nullptr, nullptr, nullptr);
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
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
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

    std::lock_guard<std::mutex> lock(mi355x::helperMutex());
    mgicp_ctx* ctx = mi355x::helperContext();
    if (!ctx)
        return -1;
    double feature_radius = 0.0;
    if (!scaledResolution(ctx, *cloud, radius_factor_, feature_radius))
        return -1;

    features->points.resize(nk);
    mgicp_fpfh_info info;
    const int rc = mgicp_fpfh_features(
        ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB), &normals->points[0].normal_x,
        sizeof(pcl::Normal), keypoints_indices->data(), nk, feature_radius, features->points[0].histogram,
        sizeof(pcl::FPFHSignature33), nullptr, nullptr, &info);
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

void InitialAlignment::obtainCorrespondences()
{
    const size_t ns = source_features_->points.size();
    const size_t nt = target_features_->points.size();
    // determineCorrespondences replaces whatever the vector held
    correspondences_->clear();
    if (ns != 0 && nt != 0)
    {
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
        if (!ctx)
            return;
        std::vector<int> match(ns);
        std::vector<float> distance(ns);
        size_t found = 0;
        int rc = mgicp_match_features(ctx, source_features_->points[0].histogram, ns, sizeof(pcl::FPFHSignature33),
                                      target_features_->points[0].histogram, nt, sizeof(pcl::FPFHSignature33),
                                      DBL_MAX, match.data(), distance.data(), &found, nullptr);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("correspondence estimation failed (%d): %s", rc, mgicp_last_error(ctx));
            return;
        }
        // PCL's output: one entry per source feature that found a target, in ascending source index.
        // pcl::Correspondence has a virtual destructor: filled field by field
        correspondences_->resize(found);
        size_t k = 0;
        for (size_t i = 0; i < ns && k < found; ++i)
        {
            if (match[i] < 0)
                continue;
            pcl::Correspondence& c = (*correspondences_)[k++];
            c.index_query = static_cast<int>(i);
            c.index_match = match[i];
            c.distance = distance[i];
        }
    }
    ROS_INFO("Found %zd correspondences", correspondences_->size());
}
