/*
 * adapter/InitialAlignment_normals_mi355x.cpp -- the NORMALS method's own steps over the MI355X engine.
 * Replaces the bodies of (src/InitialAlignment.cpp of the reference)
 *     InitialAlignment::obtainNormalsCluster      (:130-161: pcl::extractEuclideanClusters(cloud, normals, 0.05f,
 *                          tree, clusters, 20 degrees, (int)n * 0.025) over a fresh kd-tree, and the fallback
 *                          of one cluster 0 .. n - 1 when none is found; runNormalsBasedAlgorithm calls it on
 *                          both clouds without their boundary points)
 *     InitialAlignment::obtainDominantNormals     (:163-187: per cluster the normalised sum of its normals,
 *                          the first member counted twice)
 * The reference's call of Utils::onePointCloud in obtainNormalsCluster fills a cloud nothing reads: it is gone.
 * getTransformationFromNormals and its helpers (normalsCorrespondences, findIdx, matrixFromAngles) keep their
 * reference implementations: host arithmetic on at most 40 normals.
 * Delete the two definitions from src/InitialAlignment.cpp and add this file to the library sources
 * (INTEGRATION.md section 2).  Compiled inside the catkin workspace.
 */
#include <InitialAlignment.h>

#include <EngineContext_mi355x.h>
#include <mi355x_gicp.h>

#include <cmath>
#include <cstddef>
#include <numeric>
#include <vector>

namespace
{
static_assert(sizeof(pcl::PointXYZRGB) == 32, "PointXYZRGB record must be 32 bytes (x,y,z,pad,rgb,pad)");
static_assert(sizeof(pcl::Normal) == 32, "pcl::Normal record must be 32 bytes (normal[3], pad, curvature, pad)");

// what initial_alignment.py calls NORMALS_CLUSTER_TOLERANCE, NORMALS_CLUSTER_EPS_ANGLE and
// NORMALS_CLUSTER_PERCENTAJE: the link distance (a float in the reference), the largest angle to the seed's
// normal and the share of the records a reported cluster must hold
const float kClusterTolerance = 0.05f;
const double kClusterEpsAngle = 20.0 * (M_PI / 180.0);
const double kClusterMinShare = 0.025;
}  // namespace

void InitialAlignment::obtainNormalsCluster(PointCloudRGB::Ptr cloud,
                                            PointCloudNormal::Ptr normals,
                                            std::vector<pcl::PointIndices>& cluster_indices)
{
    const size_t n = cloud->points.size();
    // the reference's arithmetic: the normals' count as an int, times the share, truncated to unsigned
    const unsigned int min_size = static_cast<unsigned int>(static_cast<int>(normals->points.size()) * kClusterMinShare);
    ROS_INFO("Clustering normals with min cluster size: %d...", min_size);

    // PCL refuses normals that do not match the cloud: nothing is found then, as for an empty cloud
    if (n > 0 && normals->points.size() == n)
    {
        std::vector<int> labels(n), members(n);
        std::vector<size_t> first(n + 1);
        mgicp_normal_cluster_info info;
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
        const int rc = ctx ? mgicp_normal_clusters(ctx, &cloud->points[0].x, n, sizeof(pcl::PointXYZRGB),
                                                   &normals->points[0].normal_x, sizeof(pcl::Normal),
                                                   kClusterTolerance, kClusterEpsAngle, min_size, 0, labels.data(),
                                                   members.data(), first.data(), &info)
                           : MGICP_E_HIP;
        if (rc != MGICP_OK)
        {
            ROS_ERROR("normal clustering failed (%d): %s", rc, ctx ? mgicp_last_error(ctx) : "no engine");
        }
        else
        {
            const size_t found = static_cast<size_t>(info.n_clusters), before = cluster_indices.size();
            cluster_indices.resize(before + found);
            for (size_t c = 0; c < found; ++c)
                cluster_indices[before + c].indices.assign(members.begin() + static_cast<std::ptrdiff_t>(first[c]),
                                                           members.begin() + static_cast<std::ptrdiff_t>(first[c + 1]));
        }
    }
    ROS_INFO("Clusters found: %zd", cluster_indices.size());

    if (cluster_indices.empty())
    {
        // the reference's answer to an empty result: every record of the cloud as one cluster
        ROS_ERROR("Failed to obtain normals cluster");
        cluster_indices.resize(1);
        cluster_indices[0].indices.resize(n);
        std::iota(cluster_indices[0].indices.begin(), cluster_indices[0].indices.end(), 0);
    }
}

void InitialAlignment::obtainDominantNormals(PointCloudNormal::Ptr normals,
                                             std::vector<pcl::PointIndices> cluster_indices,
                                             PointCloudNormal::Ptr dominant_normals)
{
    const size_t nc = cluster_indices.size();
    if (nc == 0)
        return;
    // the clusters' members end to end, and where each cluster begins
    std::vector<int> members;
    std::vector<size_t> first(nc + 1, 0);
    for (size_t c = 0; c < nc; ++c)
    {
        members.insert(members.end(), cluster_indices[c].indices.begin(), cluster_indices[c].indices.end());
        first[c + 1] = members.size();
    }
    std::vector<float> xyz(3 * nc);
    {
        std::lock_guard<std::mutex> lock(mi355x::helperMutex());
        mgicp_ctx* ctx = mi355x::helperContext();
        if (!ctx)
            return;
        const int rc = mgicp_dominant_normals(ctx, normals->points.empty() ? nullptr : &normals->points[0].normal_x,
                                              normals->points.size(), sizeof(pcl::Normal), members.data(),
                                              first.data(), nc, xyz.data(), nullptr);
        if (rc != MGICP_OK)
        {
            // an empty cluster or an index outside the normals: the reference reads past its vectors there
            ROS_ERROR("dominant normals failed (%d): %s", rc, mgicp_last_error(ctx));
            return;
        }
    }
    // one record per cluster after whatever the output cloud already holds
    const size_t before = dominant_normals->points.size();
    dominant_normals->points.resize(before + nc);
    for (size_t c = 0; c < nc; ++c)
    {
        pcl::Normal& out = dominant_normals->points[before + c];
        out.normal_x = xyz[3 * c];
        out.normal_y = xyz[3 * c + 1];
        out.normal_z = xyz[3 * c + 2];
    }
}
