/*
 * TEST INFRASTRUCTURE ONLY -- drives the adapter's Utils::getNormals (adapter/Utils_mi355x.cpp) the way
 * InitialAlignment's constructor does (two clouds' resolutions, normal_radius = (res + res) * 10 for one
 * cloud aligned with itself), or at a radius given on the command line.
 *
 * usage: replay_test_normals <cloud.bin: packed float32 xyz> <normals.bin: out> [radius]
 * output lines:  "<check> ok|FAIL",  "radius <%.17g>",  "normals <count> width <w> height <h> dense <0|1>"
 * normals.bin receives the pcl::Normal records (32 bytes each) as they stand in memory.
 * exit status: 0 when every check passed.
 */
#include <Utils.h>

#include <cstdio>
#include <cstdlib>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

static int g_fail = 0;

static void check(bool ok, const char* what)
{
    std::printf("%s %s\n", what, ok ? "ok" : "FAIL");
    if (!ok)
        ++g_fail;
}

int main(int argc, char** argv)
{
    if (argc < 3)
    {
        std::fprintf(stderr, "usage: %s cloud.bin normals.bin [radius]\n", argv[0]);
        return 2;
    }
    PointCloudRGB::Ptr cloud(new PointCloudRGB);
    if (FILE* f = std::fopen(argv[1], "rb"))
    {
        float xyz[3];
        pcl::PointXYZRGB p;
        while (std::fread(xyz, sizeof(float), 3, f) == 3)
        {
            p.x = xyz[0];
            p.y = xyz[1];
            p.z = xyz[2];
            cloud->push_back(p);
        }
        std::fclose(f);
    }
    else
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    double radius = 0.0;
    if (argc > 3)
    {
        radius = std::atof(argv[3]);
    }
    else
    {
        const double res = Utils::computeCloudResolution(cloud);
        radius = (res + res) * 10;
    }
    std::printf("radius %.17g\n", radius);
    PointCloudNormal::Ptr normals(new PointCloudNormal);
    const bool ok = Utils::getNormals(cloud, radius, normals);
    check(ok, "getNormals_success");
    check(normals->points.size() == cloud->points.size(), "getNormals_size");
    check(static_cast<std::size_t>(normals->width) * normals->height == normals->points.size(), "getNormals_organised");
    bool pads = true, any_nan = false;
    for (std::size_t i = 0; i < normals->points.size(); ++i)
    {
        const pcl::Normal& q = normals->points[i];
        pads = pads && q.data_n[3] == 0.f && q.data_c[1] == 0.f && q.data_c[2] == 0.f && q.data_c[3] == 0.f;
        any_nan = any_nan || q.normal_x != q.normal_x || q.normal_y != q.normal_y || q.normal_z != q.normal_z;
    }
    check(pads, "getNormals_pads_zero");
    check(normals->is_dense == !any_nan, "getNormals_is_dense");
    std::printf("normals %zu width %u height %u dense %d\n", normals->points.size(), normals->width, normals->height,
                normals->is_dense ? 1 : 0);
    if (FILE* f = std::fopen(argv[2], "wb"))
    {
        if (!normals->points.empty())
            std::fwrite(normals->points.data(), sizeof(pcl::Normal), normals->points.size(), f);
        std::fclose(f);
    }
    else
    {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
