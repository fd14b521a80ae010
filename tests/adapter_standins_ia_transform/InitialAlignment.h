/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/InitialAlignment.h for
 * adapter/InitialAlignment_transform_mi355x.cpp: the class with the three private members that adapter
 * defines (the reference's signatures), the members they read and write -- source_keypoints_,
 * target_keypoints_, correspondences_, rigid_tf_, transform_exists_ -- and a friend through which the replay
 * driver reaches them.  <Utils.h> is tests/adapter_standins/Utils.h (pcl::PointCloud, Eigen::Matrix4f, the
 * ROS log macros); pcl::Correspondence has PCL 1.8.1's fields, default values and virtual destructor (so it
 * is not trivially copyable, as in PCL).  This directory comes first on the include path, so
 * <InitialAlignment.h> is this file.
 */
#pragma once

#include <Utils.h>

#include <limits>
#include <memory>
#include <vector>

namespace pcl
{
struct Correspondence
{
    int index_query;
    int index_match;
    union {
        float distance;
        float weight;
    };
    Correspondence() : index_query(0), index_match(-1), distance(std::numeric_limits<float>::max()) {}
    Correspondence(int q, int m, float d) : index_query(q), index_match(m), distance(d) {}
    virtual ~Correspondence() {}
};
typedef std::vector<Correspondence> Correspondences;
typedef std::shared_ptr<Correspondences> CorrespondencesPtr;
}  // namespace pcl

struct InitialAlignmentReplay;

class InitialAlignment
{
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;

public:
    InitialAlignment()
      : transform_exists_(false), rigid_tf_(Eigen::Matrix4f::Identity()), target_keypoints_(new PointCloudRGB),
        source_keypoints_(new PointCloudRGB), correspondences_(new pcl::Correspondences)
    {
    }

private:
    friend struct InitialAlignmentReplay;
    bool transform_exists_;
    Eigen::Matrix4f rigid_tf_;
    PointCloudRGB::Ptr target_keypoints_;
    PointCloudRGB::Ptr source_keypoints_;
    pcl::CorrespondencesPtr correspondences_;
    void rejectCorrespondences();
    void rejectOneToOneCorrespondences();
    void estimateTransform();
};
