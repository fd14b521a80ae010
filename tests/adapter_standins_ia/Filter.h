/*
 * TEST INFRASTRUCTURE ONLY -- stand-in of the reference's include/Filter.h for
 * adapter/InitialAlignment_mi355x.cpp: the one static member that adapter calls, with the
 * reference's signature.  Its stand-in body (Filter_standin.cpp) does what pcl::ExtractIndices does
 * there: the output becomes the indexed points, in the order of the indices.  <Utils.h> is
 * tests/adapter_standins_normals/Utils.h; pcl::IndicesPtr is a shared pointer to std::vector<int> as in
 * PCL.  This directory comes first on the include path, so <Filter.h> is this file.
 */
#pragma once

#include <Utils.h>

#include <memory>
#include <vector>

namespace pcl
{
typedef std::shared_ptr<std::vector<int>> IndicesPtr;
}

class Filter
{
    typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;

public:
    static void extractIndices(PointCloudRGB::Ptr cloud_in, PointCloudRGB::Ptr cloud_out, pcl::IndicesPtr indices);
};
