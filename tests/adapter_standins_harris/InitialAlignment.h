/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/InitialAlignment.h for
 * adapter/InitialAlignment_harris_mi355x.cpp: the class with the one private member the adapter defines
 * (the reference's signature), the radius_factor_ it reads, and a friend through which the replay driver
 * reaches both.  <Filter.h> is the stand-in beside this file (it brings pcl::IndicesPtr and, through
 * tests/adapter_standins_normals/Utils.h, the layout-exact pcl::Normal).  This directory comes first on
 * the include path, so <InitialAlignment.h> is this file.
 */
#pragma once

#include <Filter.h>

struct InitialAlignmentReplay;

class InitialAlignment
{
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
    typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

public:
    InitialAlignment() : radius_factor_(1.4) {}

private:
    friend struct InitialAlignmentReplay;
    double radius_factor_;
    int obtainHarrisKeypoints(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                              PointCloudRGB::Ptr keypoints_cloud, pcl::IndicesPtr keypoints_indices);
};
