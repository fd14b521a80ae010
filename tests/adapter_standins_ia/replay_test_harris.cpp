/*
 * TEST INFRASTRUCTURE ONLY -- drives the adapter's InitialAlignment::obtainHarrisKeypoints
 * (adapter/InitialAlignment_mi355x.cpp) as runKeypointsBasedAlgorithm does: a cloud, its normals, a keypoint
 * cloud and an index list.
 *
 * usage: replay_test_harris <cloud.bin: packed float32 xyz> <normals.bin: packed float32 nx ny nz>
 *                           <radius_factor> <keypoints.bin: out, int32>
 * output lines:  "<check> ok|FAIL",  "keypoints <count> status <rc>"
 * exit status: 0 when every check passed.
 */
#include <InitialAlignment.h>

#include <cstdio>
#include <cstdlib>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

struct InitialAlignmentReplay
{
    static int harris(InitialAlignment& ia, double radius_factor, PointCloudRGB::Ptr cloud,
                      PointCloudNormal::Ptr normals, PointCloudRGB::Ptr keypoints, pcl::IndicesPtr kidx)
    {
        ia.radius_factor_ = radius_factor;
        return ia.obtainHarrisKeypoints(cloud, normals, keypoints, kidx);
    }
};

static int g_fail = 0;

static void check(bool ok, const char* what)
{
    std::printf("%s %s\n", what, ok ? "ok" : "FAIL");
    if (!ok)
        ++g_fail;
}

static bool read_triples(const char* path, std::vector<float>& out)
{
    FILE* f = std::fopen(path, "rb");
    if (!f)
        return false;
    float v[3];
    while (std::fread(v, sizeof(float), 3, f) == 3)
        out.insert(out.end(), v, v + 3);
    std::fclose(f);
    return true;
}

static bool write_ints(const char* path, const std::vector<int>& v)
{
    FILE* f = std::fopen(path, "wb");
    if (!f)
        return false;
    if (!v.empty())
        std::fwrite(v.data(), sizeof(int), v.size(), f);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        std::fprintf(stderr, "usage: %s cloud.bin normals.bin radius_factor keypoints.bin\n", argv[0]);
        return 2;
    }
    std::vector<float> xyz, nrm;
    if (!read_triples(argv[1], xyz) || !read_triples(argv[2], nrm))
    {
        std::fprintf(stderr, "cannot read %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    const double radius_factor = std::atof(argv[3]);
    PointCloudRGB::Ptr cloud(new PointCloudRGB);
    PointCloudNormal::Ptr normals(new PointCloudNormal);
    for (std::size_t i = 0; i + 2 < xyz.size(); i += 3)
    {
        pcl::PointXYZRGB p;
        p.x = xyz[i];
        p.y = xyz[i + 1];
        p.z = xyz[i + 2];
        cloud->push_back(p);
    }
    for (std::size_t i = 0; i + 2 < nrm.size(); i += 3)
    {
        pcl::Normal q;
        q.normal_x = nrm[i];
        q.normal_y = nrm[i + 1];
        q.normal_z = nrm[i + 2];
        q.curvature = 0.25f;  // bytes between the normals the engine must step over
        normals->push_back(q);
    }
    InitialAlignment ia;

    // normals that do not match the cloud: -1, nothing written
    {
        PointCloudNormal::Ptr fewer(new PointCloudNormal(*normals));
        if (!fewer->points.empty())
            fewer->points.pop_back();
        PointCloudRGB::Ptr kp(new PointCloudRGB);
        pcl::IndicesPtr ki(new std::vector<int>);
        const int rc = InitialAlignmentReplay::harris(ia, radius_factor, cloud, fewer, kp, ki);
        check(cloud->points.empty() || (rc == -1 && kp->points.empty() && ki->empty()), "size_mismatch_is_minus_one");
    }

    PointCloudRGB::Ptr keypoints(new PointCloudRGB);
    pcl::IndicesPtr kidx(new std::vector<int>);
    const int rc = InitialAlignmentReplay::harris(ia, radius_factor, cloud, normals, keypoints, kidx);
    check(rc == (kidx->empty() ? -1 : 0), "status_follows_keypoints");
    bool same = keypoints->points.size() == kidx->size(), ascending = true;
    for (std::size_t j = 0; same && j < kidx->size(); ++j)
    {
        const pcl::PointXYZRGB& a = keypoints->points[j];
        const pcl::PointXYZRGB& b = cloud->points[static_cast<std::size_t>((*kidx)[j])];
        same = a.x == b.x && a.y == b.y && a.z == b.z;
        ascending = ascending && (j == 0 || (*kidx)[j - 1] < (*kidx)[j]);
    }
    check(same, "keypoints_are_the_indexed_points");
    check(ascending, "keypoint_indices_ascend");
    std::printf("keypoints %zu status %d\n", kidx->size(), rc);
    if (!write_ints(argv[4], *kidx))
    {
        std::fprintf(stderr, "cannot write %s\n", argv[4]);
        return 2;
    }
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
