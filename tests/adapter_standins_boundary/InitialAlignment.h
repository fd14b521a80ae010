/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/InitialAlignment.h for
 * adapter/InitialAlignment_mi355x.cpp: the class with the one private member the adapter defines
 * (the reference's signature) and a friend through which the replay driver reaches it.  <Utils.h> is
 * tests/adapter_standins_normals/Utils.h (the layout-exact pcl::Normal); pcl::IndicesPtr is a shared
 * pointer to std::vector<int> as in PCL.  This directory comes first on the include path, so
 * <InitialAlignment.h> is this file.
 */
#pragma once

#include <Utils.h>

#include <memory>
#include <vector>

namespace pcl
{
typedef std::shared_ptr<std::vector<int>> IndicesPtr;
}

struct InitialAlignmentReplay;

class InitialAlignment
{
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
    typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

public:
    InitialAlignment() {}

private:
    friend struct InitialAlignmentReplay;
    int obtainBoundaryKeypoints(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                                PointCloudRGB::Ptr keypoints_cloud, pcl::IndicesPtr keypoints_indices,
                                pcl::IndicesPtr non_keypoints_indices);
};
