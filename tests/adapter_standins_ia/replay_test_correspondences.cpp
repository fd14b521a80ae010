/*
 * TEST INFRASTRUCTURE ONLY -- drives the adapter's InitialAlignment::obtainCorrespondences
 * (adapter/InitialAlignment_mi355x.cpp) as runKeypointsBasedAlgorithm does: the two feature clouds in
 * place and a correspondence vector that already holds entries.
 *
 * usage: replay_test_correspondences <source.bin: 33 float32 per feature> <target.bin: the same>
 *                                    <query.bin: out, int32> <match.bin: out, int32> <distance.bin: out, float32>
 * output lines:  "<check> ok|FAIL",  "correspondences <count>"
 * exit status: 0 when every check passed.
 */
#include <InitialAlignment.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

typedef pcl::PointCloud<pcl::FPFHSignature33> PointCloudFPFH;

static_assert(!std::is_trivially_copyable<pcl::Correspondence>::value, "the stand-in keeps PCL's virtual destructor");

struct InitialAlignmentReplay
{
    static void fill(PointCloudFPFH::Ptr cloud, const std::vector<float>& v)
    {
        cloud->points.clear();
        for (std::size_t i = 0; i + 32 < v.size(); i += 33)
        {
            pcl::FPFHSignature33 f;
            for (int b = 0; b < 33; ++b)
                f.histogram[b] = v[i + b];
            cloud->push_back(f);
        }
    }
    static void setFeatures(InitialAlignment& ia, const std::vector<float>& src, const std::vector<float>& tgt)
    {
        fill(ia.source_features_, src);
        fill(ia.target_features_, tgt);
    }
    static pcl::Correspondences& correspondences(InitialAlignment& ia) { return *ia.correspondences_; }
    static std::size_t sourceSize(const InitialAlignment& ia) { return ia.source_features_->points.size(); }
    static std::size_t targetSize(const InitialAlignment& ia) { return ia.target_features_->points.size(); }
    static void run(InitialAlignment& ia) { ia.obtainCorrespondences(); }
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
static bool write_all(const char* path, const std::vector<T>& v)
{
    FILE* f = std::fopen(path, "wb");
    if (!f)
        return false;
    const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 6)
    {
        std::fprintf(stderr, "usage: %s source.bin target.bin query.bin match.bin distance.bin\n", argv[0]);
        return 2;
    }
    std::vector<float> src, tgt;
    if (!read_all(argv[1], src) || !read_all(argv[2], tgt))
    {
        std::fprintf(stderr, "cannot read %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    InitialAlignment ia;

    // no target feature: no correspondence, and what the vector held is gone
    {
        InitialAlignmentReplay::setFeatures(ia, src, std::vector<float>());
        InitialAlignmentReplay::correspondences(ia).push_back(pcl::Correspondence(7, 7, 7.f));
        InitialAlignmentReplay::run(ia);
        check(InitialAlignmentReplay::correspondences(ia).empty(), "no_target_gives_none");
    }

    // the call itself, on a vector that already holds two entries (determineCorrespondences replaces them)
    InitialAlignmentReplay::setFeatures(ia, src, tgt);
    pcl::Correspondences& corr = InitialAlignmentReplay::correspondences(ia);
    corr.push_back(pcl::Correspondence(7, 7, 7.f));
    corr.push_back(pcl::Correspondence());
    InitialAlignmentReplay::run(ia);
    const std::size_t ns = InitialAlignmentReplay::sourceSize(ia), nt = InitialAlignmentReplay::targetSize(ia);
    check(corr.size() <= ns, "at_most_one_per_source_feature");
    bool ascending = true, in_range = true, finite = true;
    for (std::size_t k = 0; k < corr.size(); ++k)
    {
        ascending = ascending && (k == 0 || corr[k].index_query > corr[k - 1].index_query);
        in_range = in_range && corr[k].index_query >= 0 && static_cast<std::size_t>(corr[k].index_query) < ns &&
                   corr[k].index_match >= 0 && static_cast<std::size_t>(corr[k].index_match) < nt;
        finite = finite && corr[k].distance >= 0.f && corr[k].distance < std::numeric_limits<float>::max();
    }
    check(ascending, "ascending_index_query");
    check(in_range, "indices_in_range");
    check(finite, "distances_below_flt_max");
    std::printf("correspondences %zu\n", corr.size());
    std::vector<int> q, m;
    std::vector<float> d;
    for (std::size_t k = 0; k < corr.size(); ++k)
    {
        q.push_back(corr[k].index_query);
        m.push_back(corr[k].index_match);
        d.push_back(corr[k].distance);
    }
    if (!write_all(argv[3], q) || !write_all(argv[4], m) || !write_all(argv[5], d))
    {
        std::fprintf(stderr, "cannot write %s, %s or %s\n", argv[3], argv[4], argv[5]);
        return 2;
    }
    check(ros::error_count() == 0, "no_error_logged");
    return g_fail ? 1 : 0;
}
