/*
 * TEST INFRASTRUCTURE ONLY -- minimal stand-in of pcl::PointIndices (pcl/PointIndices.h): a header
 * and the vector of point indices, which is all the adapter fills.
 */
#pragma once

#include "standin_deps.h"

namespace pcl
{
struct PointIndices
{
    PCLHeader header;
    std::vector<int> indices;
};
}  // namespace pcl
