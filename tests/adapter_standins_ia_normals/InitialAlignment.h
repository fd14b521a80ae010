/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/InitialAlignment.h for
 * adapter/InitialAlignment_normals_mi355x.cpp: the class with the two private members that adapter defines
 * (the reference's signatures) and a friend through which the replay driver reaches them.  <Utils.h> is
 * tests/adapter_standins_normals/Utils.h (pcl::PointCloud, the layout-exact pcl::Normal, the ROS log macros);
 * pcl::PointIndices is a header and the vector of point indices, with PCL's Ptr.  This directory comes first on
 * the include path, so <InitialAlignment.h> is this file.
 */
#pragma once

#include <Utils.h>

#include <memory>
#include <vector>

namespace pcl
{
struct PointIndices
{
    typedef std::shared_ptr<PointIndices> Ptr;
    PCLHeader header;
    std::vector<int> indices;
};
}  // namespace pcl

struct InitialAlignmentReplay;

class InitialAlignment
{
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
    typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

public:
    InitialAlignment() {}

private:
    friend struct InitialAlignmentReplay;
    void obtainNormalsCluster(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                              std::vector<pcl::PointIndices>& cluster_indices);
    void obtainDominantNormals(PointCloudNormal::Ptr normals, std::vector<pcl::PointIndices> cluster_indices,
                               PointCloudNormal::Ptr dominant_normals);
};
