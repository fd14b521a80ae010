/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/InitialAlignment.h for
 * adapter/InitialAlignment_features_mi355x.cpp: the class with the one private member the adapter defines
 * (the reference's signature), the radius_factor_ it reads, and a friend through which the replay driver
 * reaches both.  <Utils.h> is tests/adapter_standins_normals/Utils.h (the layout-exact pcl::Normal);
 * pcl::FPFHSignature33 is PCL's 33 floats; pcl::IndicesPtr is a shared pointer to std::vector<int> as in
 * PCL.  This directory comes first on the include path, so <InitialAlignment.h> is this file.
 */
#pragma once

#include <Utils.h>

#include <memory>
#include <vector>

namespace pcl
{
typedef std::shared_ptr<std::vector<int>> IndicesPtr;

struct FPFHSignature33
{
    float histogram[33];
    static int descriptorSize() { return 33; }
};
}  // namespace pcl

struct InitialAlignmentReplay;

class InitialAlignment
{
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
    typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;
    typedef pcl::PointCloud<pcl::FPFHSignature33> PointCloudFPFH;

public:
    InitialAlignment() : radius_factor_(1.4) {}

private:
    friend struct InitialAlignmentReplay;
    double radius_factor_;
    int obtainFeatures(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals, pcl::IndicesPtr keypoints_indices,
                       PointCloudFPFH::Ptr features);
};
