/*
 * TEST INFRASTRUCTURE ONLY -- the FODDetector members the adapter does NOT replace (in the catkin
 * package they stay in src/FODDetector.cpp), restated for the replay: tolerance 0 falls back to
 * 4e-3 with a warning, the minimum size is stored as given, and each cluster becomes a cloud of
 * copies of its records in index order.
 */
#include <FODDetector.h>

FODDetector::FODDetector(PointCloudRGB::Ptr cloud, double cluster_tolerance, double min_fod_points) : cloud_(cloud)
{
    setClusterTolerance(cluster_tolerance);
    setMinFODpoints(min_fod_points);
}

void FODDetector::setClusterTolerance(double tolerance)
{
    if (tolerance == 0)
        ROS_WARN("FODDetector: invalid tolerance value: %f", tolerance);
    cluster_tolerance_ = tolerance == 0 ? 4e-3 : tolerance;
}

void FODDetector::setMinFODpoints(double min_fod_points)
{
    min_cluster_size_ = min_fod_points;
}

void FODDetector::getFODIndices(std::vector<pcl::PointIndices>& fod_indices)
{
    fod_indices = cluster_indices_;
}

int FODDetector::fodIndicesToPointCloud(std::vector<PointCloudRGB::Ptr>& cloud_array)
{
    for (const pcl::PointIndices& c : cluster_indices_)
    {
        PointCloudRGB::Ptr out(new PointCloudRGB);
        for (int i : c.indices)
            out->push_back(cloud_->points[static_cast<std::size_t>(i)]);
        out->is_dense = true;
        cloud_array.push_back(out);
    }
    return static_cast<int>(cluster_indices_.size());
}
