/*
 * TEST INFRASTRUCTURE ONLY -- replay of the reference's test/test_fod_detector.cpp cases
 * testFODClustering and testEmptyCloud through the adapter's FODDetector::clusterPossibleFODs
 * (gtest is not needed: one line per check).
 *
 * output lines:  "<check> ok|FAIL"  and  "cluster <rank> size <points> first <smallest index>"
 * exit status: 0 when every check passed.
 */
#include <FODDetector.h>

#include <cstdio>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;

static int g_fail = 0;

static void check(bool ok, const char* what)
{
    std::printf("%s %s\n", what, ok ? "ok" : "FAIL");
    if (!ok)
        ++g_fail;
}

// a lattice cube of edge `dim` at (pos, pos, pos): fp32 loop counters stepping by `step`
static void addCube(PointCloudRGB& cloud, float pos, float dim, float step)
{
    pcl::PointXYZRGB p;
    p.r = p.g = p.b = 255;
    for (float i = pos; i < pos + dim; i += step)
        for (float j = pos; j < pos + dim; j += step)
            for (float k = pos; k < pos + dim; k += step)
            {
                p.x = i;
                p.y = j;
                p.z = k;
                cloud.push_back(p);
            }
}

int main()
{
    const int min_fod_points = 3;
    const double th = 4e-3 * 3;
    {
        PointCloudRGB::Ptr cloud(new PointCloudRGB);
        addCube(*cloud, 0.f, 3.f, 0.1f);
        addCube(*cloud, 10.f, 3.f, 0.1f);
        addCube(*cloud, 20.f, 3.f, 0.1f);
        std::printf("points %zu\n", cloud->size());
        FODDetector det(cloud, th * 10, min_fod_points);
        det.clusterPossibleFODs();
        std::vector<PointCloudRGB::Ptr> fods;
        const int n = det.fodIndicesToPointCloud(fods);
        check(n == 3, "testFODClustering_count");
        check(fods.size() == 3, "testFODClustering_clouds");
        std::vector<pcl::PointIndices> idx;
        det.getFODIndices(idx);
        bool ascending = true, copies = idx.size() == fods.size();
        for (std::size_t c = 0; c < idx.size(); ++c)
        {
            std::printf("cluster %zu size %zu first %d\n", c, idx[c].indices.size(),
                        idx[c].indices.empty() ? -1 : idx[c].indices[0]);
            for (std::size_t m = 1; m < idx[c].indices.size(); ++m)
                ascending = ascending && idx[c].indices[m - 1] < idx[c].indices[m];
            copies = copies && c < fods.size() && fods[c]->size() == idx[c].indices.size();
            if (copies && !idx[c].indices.empty())
                copies = fods[c]->points[0].x == cloud->points[static_cast<std::size_t>(idx[c].indices[0])].x;
        }
        check(ascending, "testFODClustering_ascending");
        check(copies, "testFODClustering_copies");
    }
    {
        PointCloudRGB::Ptr empty(new PointCloudRGB);
        FODDetector det(empty, th * 10, min_fod_points);
        det.clusterPossibleFODs();
        std::vector<PointCloudRGB::Ptr> fods;
        const int n = det.fodIndicesToPointCloud(fods);
        check(n == 0, "testEmptyCloud_count");
        check(fods.empty(), "testEmptyCloud_clouds");
    }
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
