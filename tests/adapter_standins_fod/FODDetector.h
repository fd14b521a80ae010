/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/FODDetector.h: the same class name,
 * member signatures and private fields the adapter (adapter/FODDetector_mi355x.cpp) and the replay
 * use, over the stand-ins of tests/adapter_standins plus pcl::PointIndices (PointIndices.h here).
 */
#pragma once

#include <Utils.h>

#include "PointIndices.h"

class FODDetector
{
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;

public:
    FODDetector(PointCloudRGB::Ptr cloud, double cluster_tolerance, double min_fod_points);
    ~FODDetector() {}

    void setClusterTolerance(double tolerance);
    void setMinFODpoints(double min_fod_points);
    void clusterPossibleFODs();
    void getFODIndices(std::vector<pcl::PointIndices>& fod_indices);
    int fodIndicesToPointCloud(std::vector<PointCloudRGB::Ptr>& cloud_array);

private:
    double cluster_tolerance_;
    double min_cluster_size_;
    PointCloudRGB::Ptr cloud_;
    std::vector<pcl::PointIndices> cluster_indices_;
};
