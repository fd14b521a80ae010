/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/Utils.h for adapter/Utils_mi355x.cpp:
 * the members of tests/adapter_standins/Utils.h (whose definitions, Utils_standin.cpp, are linked in) plus
 * getNormals with the reference's signature (its include/Utils.h:36,68), and a layout-exact
 * pcl::Normal (PCL 1.8 PCL_ADD_NORMAL4D + curvature: 32 bytes, 16-byte aligned, normal_x/y/z at 0/4/8,
 * data_n[3] at 12, curvature at 16).  This directory comes first on the include path, so <Utils.h> is
 * this file.
 */
#pragma once

#include "standin_deps.h"

namespace pcl
{
struct alignas(16) Normal
{
    union {
        float data_n[4];
        float normal[3];
        struct
        {
            float normal_x, normal_y, normal_z;
        };
    };
    union {
        struct
        {
            float curvature;
        };
        float data_c[4];
    };
    Normal() : data_n{0.f, 0.f, 0.f, 0.f}, data_c{0.f, 0.f, 0.f, 0.f} {}
};
}  // namespace pcl

class Utils
{
    typedef pcl::PointCloud<pcl::PointXYZ> PointCloudXYZ;
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
    typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

public:
    Utils() = delete;
    static bool getNormals(PointCloudRGB::Ptr& cloud, double normal_radius, PointCloudNormal::Ptr& normals);
    static bool isValidCloud(PointCloudRGB::Ptr cloud);
    static bool isValidTransform(Eigen::Matrix4f transform);
    static void cloudToROSMsg(PointCloudRGB::Ptr cloud, sensor_msgs::PointCloud2& cloud_msg,
                              const std::string& frameid = "world");
    static double computeCloudResolution(PointCloudRGB::Ptr cloud);
    static void printTransform(const Eigen::Matrix4f& transform);
};
