/*
 * TEST INFRASTRUCTURE ONLY -- drives the adapter's InitialAlignment::obtainBoundaryKeypoints
 * (adapter/InitialAlignment_mi355x.cpp) as runKeypointsBasedAlgorithm does: a cloud, its normals, a
 * keypoint cloud that already holds points, and the two index lists.
 *
 * usage: replay_test_boundary <cloud.bin: packed float32 xyz> <normals.bin: packed float32 nx ny nz>
 *                             <keypoints.bin: out, int32> <non_keypoints.bin: out, int32>
 * output lines:  "<check> ok|FAIL",  "keypoints <count> non_keypoints <count> status <rc>"
 * exit status: 0 when every check passed.
 */
#include <InitialAlignment.h>

#include <cstdio>
#include <cstdlib>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

struct InitialAlignmentReplay
{
    static int boundary(InitialAlignment& ia, PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                        PointCloudRGB::Ptr keypoints, pcl::IndicesPtr kidx, pcl::IndicesPtr nidx)
    {
        return ia.obtainBoundaryKeypoints(cloud, normals, keypoints, kidx, nidx);
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
        std::fprintf(stderr, "usage: %s cloud.bin normals.bin keypoints.bin non_keypoints.bin\n", argv[0]);
        return 2;
    }
    std::vector<float> xyz, nrm;
    if (!read_triples(argv[1], xyz) || !read_triples(argv[2], nrm))
    {
        std::fprintf(stderr, "cannot read %s or %s\n", argv[1], argv[2]);
        return 2;
    }
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

    // normals that do not match the cloud: -1, nothing appended
    {
        PointCloudNormal::Ptr fewer(new PointCloudNormal(*normals));
        if (!fewer->points.empty())
            fewer->points.pop_back();
        PointCloudRGB::Ptr kp(new PointCloudRGB);
        pcl::IndicesPtr ki(new std::vector<int>), ni(new std::vector<int>);
        const int rc = InitialAlignmentReplay::boundary(ia, cloud, fewer, kp, ki, ni);
        check(cloud->points.empty() || (rc == -1 && kp->points.empty() && ki->empty() && ni->empty()),
              "size_mismatch_is_minus_one");
    }

    // the call itself, on a keypoint cloud that already holds two points
    PointCloudRGB::Ptr keypoints(new PointCloudRGB);
    pcl::PointXYZRGB old0, old1;
    old0.x = 101.f;
    old1.x = 102.f;
    keypoints->points.push_back(old0);
    keypoints->points.push_back(old1);
    pcl::IndicesPtr kidx(new std::vector<int>), nidx(new std::vector<int>);
    const int rc = InitialAlignmentReplay::boundary(ia, cloud, normals, keypoints, kidx, nidx);
    check(rc == (kidx->empty() ? -1 : 0), "status_follows_keypoints");
    check(kidx->size() + nidx->size() == cloud->points.size(), "every_record_listed_once");
    check(keypoints->points.size() == 2 + kidx->size() && keypoints->points[0].x == 101.f &&
              keypoints->points[1].x == 102.f,
          "keypoints_cloud_keeps_old_points");
    bool same = keypoints->points.size() == 2 + kidx->size(), ascending = true;
    for (std::size_t j = 0; same && j < kidx->size(); ++j)
    {
        const pcl::PointXYZRGB& a = keypoints->points[2 + j];
        const pcl::PointXYZRGB& b = cloud->points[(*kidx)[j]];
        same = a.x == b.x && a.y == b.y && a.z == b.z;
        ascending = ascending && (j == 0 || (*kidx)[j - 1] < (*kidx)[j]);
    }
    check(same, "keypoints_are_the_indexed_points");
    check(ascending, "keypoint_indices_ascend");
    std::printf("keypoints %zu non_keypoints %zu status %d\n", kidx->size(), nidx->size(), rc);
    if (!write_ints(argv[3], *kidx) || !write_ints(argv[4], *nidx))
    {
        std::fprintf(stderr, "cannot write %s or %s\n", argv[3], argv[4]);
        return 2;
    }
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
