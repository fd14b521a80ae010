/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/InitialAlignment.h for
 * adapter/InitialAlignment_mi355x.cpp: the class with the four private members the adapter defines (the
 * reference's signatures), the radius_factor_ it reads, the three members obtainCorrespondences reads and
 * fills, and a friend through which the replay drivers reach them.  <Filter.h> is the stand-in beside this
 * file (it brings pcl::IndicesPtr and, through tests/adapter_standins_normals/Utils.h, pcl::PointCloud, the
 * layout-exact pcl::Normal and the ROS log macros); pcl::FPFHSignature33 is PCL's 33 floats;
 * pcl::Correspondence has PCL 1.8.1's fields, default values and virtual destructor (so it is not trivially
 * copyable, as in PCL), pcl::Correspondences is a vector of them and pcl::CorrespondencesPtr a shared
 * pointer to it.  This directory comes first on the include path, so <InitialAlignment.h> is this file.
 */
#pragma once

#include <Filter.h>

#include <limits>
#include <memory>
#include <vector>

namespace pcl
{
struct FPFHSignature33
{
    float histogram[33];
    static int descriptorSize() { return 33; }
};

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
    typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;
    typedef pcl::PointCloud<pcl::FPFHSignature33> PointCloudFPFH;

public:
    InitialAlignment()
      : radius_factor_(1.4), target_features_(new PointCloudFPFH), source_features_(new PointCloudFPFH),
        correspondences_(new pcl::Correspondences)
    {
    }

private:
    friend struct InitialAlignmentReplay;
    double radius_factor_;
    PointCloudFPFH::Ptr target_features_;
    PointCloudFPFH::Ptr source_features_;
    pcl::CorrespondencesPtr correspondences_;
    int obtainHarrisKeypoints(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                              PointCloudRGB::Ptr keypoints_cloud, pcl::IndicesPtr keypoints_indices);
    int obtainBoundaryKeypoints(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                                PointCloudRGB::Ptr keypoints_cloud, pcl::IndicesPtr keypoints_indices,
                                pcl::IndicesPtr non_keypoints_indices);
    int obtainFeatures(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals, pcl::IndicesPtr keypoints_indices,
                       PointCloudFPFH::Ptr features);
    void obtainCorrespondences();
};
