/*
 * TEST INFRASTRUCTURE ONLY -- the stand-in body of Filter::extractIndices (the Filter.h beside this file),
 * which InitialAlignment::obtainHarrisKeypoints ends in: every replay driver of this directory links the
 * whole adapter/InitialAlignment_mi355x.cpp and so needs it.
 */
#include <Filter.h>

// pcl::ExtractIndices::filter: the output is replaced by the indexed points
void Filter::extractIndices(PointCloudRGB::Ptr cloud_in, PointCloudRGB::Ptr cloud_out, pcl::IndicesPtr indices)
{
    cloud_out->points.clear();
    for (std::size_t j = 0; j < indices->size(); ++j)
        cloud_out->points.push_back(cloud_in->points[static_cast<std::size_t>((*indices)[j])]);
    cloud_out->width = static_cast<std::uint32_t>(cloud_out->points.size());
    cloud_out->height = 1;
}
