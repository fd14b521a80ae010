/*
 * TEST INFRASTRUCTURE ONLY -- drives the adapter's InitialAlignment::rejectCorrespondences,
 * rejectOneToOneCorrespondences and estimateTransform (adapter/InitialAlignment_transform_mi355x.cpp) in the
 * order of runKeypointsBasedAlgorithm, on files of its inputs, and writes what each step leaves behind.
 *
 * usage: replay_test_transform <source_kp.bin: 3 float32 per keypoint> <target_kp.bin: the same>
 *                              <query.bin: int32> <match.bin: int32> <distance.bin: float32> <out directory>
 * files written: ransac_{query,match,distance}.bin, tf_ransac.bin (16 float32, column-major),
 *                one_{query,match,distance}.bin, tf.bin
 * output lines:  "<check> ok|FAIL",  "remaining <count>", "one_to_one <count>"
 * exit status: 0 when every check passed.
 */
#include <InitialAlignment.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;

static_assert(!std::is_trivially_copyable<pcl::Correspondence>::value, "the stand-in keeps PCL's virtual destructor");

struct InitialAlignmentReplay
{
    static void fill(PointCloudRGB::Ptr cloud, const std::vector<float>& v)
    {
        cloud->points.clear();
        for (std::size_t i = 0; i + 2 < v.size(); i += 3)
        {
            pcl::PointXYZRGB p;
            p.x = v[i];
            p.y = v[i + 1];
            p.z = v[i + 2];
            cloud->push_back(p);
        }
    }
    static void setKeypoints(InitialAlignment& ia, const std::vector<float>& src, const std::vector<float>& tgt)
    {
        fill(ia.source_keypoints_, src);
        fill(ia.target_keypoints_, tgt);
    }
    static pcl::Correspondences& correspondences(InitialAlignment& ia) { return *ia.correspondences_; }
    static const Eigen::Matrix4f& transform(const InitialAlignment& ia) { return ia.rigid_tf_; }
    static bool exists(const InitialAlignment& ia) { return ia.transform_exists_; }
    static void reject(InitialAlignment& ia) { ia.rejectCorrespondences(); }
    static void oneToOne(InitialAlignment& ia) { ia.rejectOneToOneCorrespondences(); }
    static void estimate(InitialAlignment& ia) { ia.estimateTransform(); }
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

template <class T>
static bool write_all(const std::string& path, const T* v, std::size_t n)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f)
        return false;
    const bool ok = n == 0 || std::fwrite(v, sizeof(T), n, f) == n;
    std::fclose(f);
    return ok;
}

static bool write_corr(const std::string& dir, const char* prefix, const pcl::Correspondences& corr)
{
    std::vector<int> q, m;
    std::vector<float> d;
    for (std::size_t k = 0; k < corr.size(); ++k)
    {
        q.push_back(corr[k].index_query);
        m.push_back(corr[k].index_match);
        d.push_back(corr[k].distance);
    }
    const std::string base = dir + "/" + prefix;
    return write_all(base + "_query.bin", q.data(), q.size()) && write_all(base + "_match.bin", m.data(), m.size()) &&
           write_all(base + "_distance.bin", d.data(), d.size());
}

int main(int argc, char** argv)
{
    if (argc < 7)
    {
        std::fprintf(stderr, "usage: %s source_kp.bin target_kp.bin query.bin match.bin distance.bin out_dir\n", argv[0]);
        return 2;
    }
    std::vector<float> src, tgt, dist;
    std::vector<int> query, match;
    if (!read_all(argv[1], src) || !read_all(argv[2], tgt) || !read_all(argv[3], query) || !read_all(argv[4], match) ||
        !read_all(argv[5], dist) || query.size() != match.size() || query.size() != dist.size())
    {
        std::fprintf(stderr, "cannot read the inputs\n");
        return 2;
    }
    const std::string out = argv[6];
    InitialAlignment ia;
    InitialAlignmentReplay::setKeypoints(ia, src, tgt);
    pcl::Correspondences& corr = InitialAlignmentReplay::correspondences(ia);

    // no correspondence: the rejectors leave the empty vector alone, the estimate is the identity
    InitialAlignmentReplay::reject(ia);
    InitialAlignmentReplay::oneToOne(ia);
    check(corr.empty(), "empty_stays_empty");
    InitialAlignmentReplay::estimate(ia);
    check(InitialAlignmentReplay::transform(ia) == Eigen::Matrix4f::Identity() && InitialAlignmentReplay::exists(ia),
          "empty_gives_identity");

    for (std::size_t k = 0; k < query.size(); ++k)
        corr.push_back(pcl::Correspondence(query[k], match[k], dist[k]));
    const std::size_t m = corr.size();

    InitialAlignmentReplay::reject(ia);
    check(corr.size() <= m, "ransac_removes_only");
    bool in_order = true;
    for (std::size_t k = 1; k < corr.size(); ++k)
        in_order = in_order && corr[k].index_query > corr[k - 1].index_query;
    check(in_order, "ransac_keeps_input_order");
    std::printf("remaining %zu\n", corr.size());
    bool ok = write_corr(out, "ransac", corr);
    InitialAlignmentReplay::estimate(ia);
    ok = ok && write_all(out + "/tf_ransac.bin", InitialAlignmentReplay::transform(ia).data(), 16);

    const std::size_t before = corr.size();
    InitialAlignmentReplay::oneToOne(ia);
    check(corr.size() <= before, "one_to_one_removes_only");
    bool ascending = true;
    for (std::size_t k = 1; k < corr.size(); ++k)
        ascending = ascending && corr[k].index_match > corr[k - 1].index_match;
    check(ascending, "one_to_one_ascending_match");
    std::printf("one_to_one %zu\n", corr.size());
    ok = ok && write_corr(out, "one", corr);
    InitialAlignmentReplay::estimate(ia);
    ok = ok && write_all(out + "/tf.bin", InitialAlignmentReplay::transform(ia).data(), 16);
    check(InitialAlignmentReplay::exists(ia), "transform_exists");
    if (!ok)
    {
        std::fprintf(stderr, "cannot write into %s\n", out.c_str());
        return 2;
    }
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
