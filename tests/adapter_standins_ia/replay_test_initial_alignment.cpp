/*
 * TEST INFRASTRUCTURE ONLY -- drives the four members of adapter/InitialAlignment_mi355x.cpp in one process,
 * and so on the one engine context they share (adapter/EngineContext_mi355x.h), in the order of a keypoint
 * method: obtainBoundaryKeypoints on the first cloud, obtainHarrisKeypoints on the second, obtainFeatures on
 * each of the two keypoint sets, obtainCorrespondences from the first features to the second, and then the
 * first member once more.  Every output goes to a file of the format the single-member drivers write.
 *
 * usage: replay_test_initial_alignment <cloud_a.bin> <normals_a.bin> <cloud_b.bin> <normals_b.bin>
 *                                      <radius_factor> <out_dir>
 *        (clouds: packed float32 xyz; normals: packed float32 nx ny nz)
 * files in out_dir:  boundary_kp.bin boundary_nkp.bin harris_kp.bin (int32), fpfh_boundary.bin
 *                    fpfh_harris.bin (33 float32 per keypoint), corr_query.bin corr_match.bin (int32)
 *                    corr_distance.bin (float32), boundary_again_kp.bin boundary_again_nkp.bin (int32)
 * output lines:  "<check> ok|FAIL",  "boundary <count> harris <count> correspondences <count>"
 * exit status: 0 when every check passed.
 */
#include <InitialAlignment.h>

#include <cstdio>
#include <cstdlib>
#include <string>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;
typedef pcl::PointCloud<pcl::FPFHSignature33> PointCloudFPFH;

struct InitialAlignmentReplay
{
    InitialAlignment ia;
    explicit InitialAlignmentReplay(double radius_factor) { ia.radius_factor_ = radius_factor; }
    int boundary(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals, pcl::IndicesPtr kidx, pcl::IndicesPtr nidx)
    {
        PointCloudRGB::Ptr keypoints(new PointCloudRGB);
        return ia.obtainBoundaryKeypoints(cloud, normals, keypoints, kidx, nidx);
    }
    int harris(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals, pcl::IndicesPtr kidx)
    {
        PointCloudRGB::Ptr keypoints(new PointCloudRGB);
        return ia.obtainHarrisKeypoints(cloud, normals, keypoints, kidx);
    }
    int features(PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals, pcl::IndicesPtr kidx, PointCloudFPFH::Ptr out)
    {
        return ia.obtainFeatures(cloud, normals, kidx, out);
    }
    const pcl::Correspondences& correspond(PointCloudFPFH::Ptr source, PointCloudFPFH::Ptr target)
    {
        ia.source_features_ = source;
        ia.target_features_ = target;
        ia.obtainCorrespondences();
        return *ia.correspondences_;
    }
};

static int g_fail = 0;

static void check(bool ok, const char* what)
{
    std::printf("%s %s\n", what, ok ? "ok" : "FAIL");
    if (!ok)
        ++g_fail;
}

static bool read_cloud(const char* cloud_path, const char* normals_path, PointCloudRGB::Ptr cloud,
                       PointCloudNormal::Ptr normals)
{
    FILE* f = std::fopen(cloud_path, "rb");
    if (!f)
        return false;
    float v[3];
    while (std::fread(v, sizeof(float), 3, f) == 3)
    {
        pcl::PointXYZRGB p;
        p.x = v[0];
        p.y = v[1];
        p.z = v[2];
        cloud->push_back(p);
    }
    std::fclose(f);
    if (!(f = std::fopen(normals_path, "rb")))
        return false;
    while (std::fread(v, sizeof(float), 3, f) == 3)
    {
        pcl::Normal q;
        q.normal_x = v[0];
        q.normal_y = v[1];
        q.normal_z = v[2];
        q.curvature = 0.25f;  // bytes between the normals the engine must step over
        normals->push_back(q);
    }
    std::fclose(f);
    return true;
}

static std::string g_dir;

template <class T>
static void write_all(const char* name, const std::vector<T>& v)
{
    const std::string path = g_dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    const bool ok = f && (v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
    if (f)
        std::fclose(f);
    if (!ok)
    {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        std::exit(2);
    }
}

static void write_features(const char* name, const PointCloudFPFH& features)
{
    std::vector<float> v;
    for (std::size_t k = 0; k < features.points.size(); ++k)
        v.insert(v.end(), features.points[k].histogram, features.points[k].histogram + 33);
    write_all(name, v);
}

int main(int argc, char** argv)
{
    if (argc < 7)
    {
        std::fprintf(stderr, "usage: %s cloud_a.bin normals_a.bin cloud_b.bin normals_b.bin radius_factor out_dir\n",
                     argv[0]);
        return 2;
    }
    PointCloudRGB::Ptr cloud_a(new PointCloudRGB), cloud_b(new PointCloudRGB);
    PointCloudNormal::Ptr normals_a(new PointCloudNormal), normals_b(new PointCloudNormal);
    if (!read_cloud(argv[1], argv[2], cloud_a, normals_a) || !read_cloud(argv[3], argv[4], cloud_b, normals_b))
    {
        std::fprintf(stderr, "cannot read the clouds or the normals\n");
        return 2;
    }
    InitialAlignmentReplay replay(std::atof(argv[5]));
    g_dir = argv[6];

    pcl::IndicesPtr bkp(new std::vector<int>), bnkp(new std::vector<int>), hkp(new std::vector<int>);
    check(replay.boundary(cloud_a, normals_a, bkp, bnkp) == 0, "boundary_status");
    write_all("boundary_kp.bin", *bkp);
    write_all("boundary_nkp.bin", *bnkp);
    check(replay.harris(cloud_b, normals_b, hkp) == 0, "harris_status");
    write_all("harris_kp.bin", *hkp);

    PointCloudFPFH::Ptr bfeat(new PointCloudFPFH), hfeat(new PointCloudFPFH);
    check(replay.features(cloud_a, normals_a, bkp, bfeat) == 0 && bfeat->points.size() == bkp->size(),
          "boundary_features_status");
    write_features("fpfh_boundary.bin", *bfeat);
    check(replay.features(cloud_b, normals_b, hkp, hfeat) == 0 && hfeat->points.size() == hkp->size(),
          "harris_features_status");
    write_features("fpfh_harris.bin", *hfeat);

    const pcl::Correspondences& corr = replay.correspond(bfeat, hfeat);
    std::vector<int> q, m;
    std::vector<float> d;
    for (std::size_t k = 0; k < corr.size(); ++k)
    {
        q.push_back(corr[k].index_query);
        m.push_back(corr[k].index_match);
        d.push_back(corr[k].distance);
    }
    write_all("corr_query.bin", q);
    write_all("corr_match.bin", m);
    write_all("corr_distance.bin", d);

    // the first member again, after every other call kind went through the context
    pcl::IndicesPtr bkp2(new std::vector<int>), bnkp2(new std::vector<int>);
    check(replay.boundary(cloud_a, normals_a, bkp2, bnkp2) == 0, "boundary_again_status");
    check(*bkp2 == *bkp && *bnkp2 == *bnkp, "boundary_again_is_the_first_result");
    write_all("boundary_again_kp.bin", *bkp2);
    write_all("boundary_again_nkp.bin", *bnkp2);

    std::printf("boundary %zu harris %zu correspondences %zu\n", bkp->size(), hkp->size(), corr.size());
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
