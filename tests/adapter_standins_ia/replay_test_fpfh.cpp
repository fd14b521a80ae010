/*
 * TEST INFRASTRUCTURE ONLY -- drives the adapter's InitialAlignment::obtainFeatures
 * (adapter/InitialAlignment_mi355x.cpp) as runKeypointsBasedAlgorithm does: a cloud, its normals, the
 * keypoint indices and a feature cloud that already holds records.
 *
 * usage: replay_test_fpfh <cloud.bin: packed float32 xyz> <normals.bin: packed float32 nx ny nz>
 *                         <keypoints.bin: int32> <fpfh.bin: out, 33 float32 per keypoint>
 * output lines:  "<check> ok|FAIL",  "features <count> status <rc>"
 * exit status: 0 when every check passed.
 */
#include <InitialAlignment.h>

#include <cstdio>
#include <cstdlib>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;
typedef pcl::PointCloud<pcl::FPFHSignature33> PointCloudFPFH;

struct InitialAlignmentReplay
{
    static int features(InitialAlignment& ia, PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                        pcl::IndicesPtr kidx, PointCloudFPFH::Ptr out)
    {
        return ia.obtainFeatures(cloud, normals, kidx, out);
    }
    static double radiusFactor(const InitialAlignment& ia) { return ia.radius_factor_; }
};

static int g_fail = 0;

static void check(bool ok, const char* what)
{
    std::printf("%s %s\n", what, ok ? "ok" : "FAIL");
    if (!ok)
        ++g_fail;
}

template <class T>
static bool read_all(const char* path, std::vector<T>& out)
{
    FILE* f = std::fopen(path, "rb");
    if (!f)
        return false;
    T v;
    while (std::fread(&v, sizeof(T), 1, f) == 1)
        out.push_back(v);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        std::fprintf(stderr, "usage: %s cloud.bin normals.bin keypoints.bin fpfh.bin\n", argv[0]);
        return 2;
    }
    std::vector<float> xyz, nrm;
    std::vector<int> kp;
    if (!read_all(argv[1], xyz) || !read_all(argv[2], nrm) || !read_all(argv[3], kp))
    {
        std::fprintf(stderr, "cannot read %s, %s or %s\n", argv[1], argv[2], argv[3]);
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
    pcl::IndicesPtr kidx(new std::vector<int>(kp));
    InitialAlignment ia;
    check(InitialAlignmentReplay::radiusFactor(ia) == 1.4, "radius_factor_is_the_default");

    // normals that do not match the cloud, and no keypoint: -1, no feature
    {
        PointCloudNormal::Ptr fewer(new PointCloudNormal(*normals));
        if (!fewer->points.empty())
            fewer->points.pop_back();
        PointCloudFPFH::Ptr out(new PointCloudFPFH);
        const int rc = InitialAlignmentReplay::features(ia, cloud, fewer, kidx, out);
        check(cloud->points.empty() || (rc == -1 && out->points.empty()), "size_mismatch_is_minus_one");
        pcl::IndicesPtr none(new std::vector<int>);
        const int rc0 = InitialAlignmentReplay::features(ia, cloud, normals, none, out);
        check(rc0 == -1 && out->points.empty(), "no_keypoint_is_minus_one");
    }

    // the call itself, on a feature cloud that already holds two records (compute() replaces them)
    PointCloudFPFH::Ptr features(new PointCloudFPFH);
    features->push_back(pcl::FPFHSignature33());
    features->push_back(pcl::FPFHSignature33());
    const int rc = InitialAlignmentReplay::features(ia, cloud, normals, kidx, features);
    check(rc == (kidx->empty() ? -1 : 0), "status_follows_features");
    check(features->points.size() == kidx->size() && features->width == kidx->size() &&
              features->height == (kidx->empty() ? 0u : 1u),
          "one_record_per_keypoint");
    std::printf("features %zu status %d\n", features->points.size(), rc);
    FILE* f = std::fopen(argv[4], "wb");
    if (!f)
    {
        std::fprintf(stderr, "cannot write %s\n", argv[4]);
        return 2;
    }
    for (std::size_t k = 0; k < features->points.size(); ++k)
        std::fwrite(features->points[k].histogram, sizeof(float), 33, f);
    std::fclose(f);
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
