/*
 * TEST INFRASTRUCTURE ONLY -- drives the adapter's InitialAlignment::obtainNormalsCluster and
 * obtainDominantNormals (adapter/InitialAlignment_normals_mi355x.cpp) as runNormalsBasedAlgorithm does: a cloud
 * and its normals, the clusters, then their dominant normals.
 *
 * usage: replay_test_normals_cluster <cloud.bin: packed float32 xyz> <normals.bin: packed float32 nx ny nz>
 *                                    <indices.bin: out, int32> <sizes.bin: out, int32> <dominant.bin: out, float32 x 3>
 * output lines:  "<check> ok|FAIL",  "clusters <count> clustered <count>"
 * exit status: 0 when every check passed.
 */
#include <InitialAlignment.h>

#include <cstdio>
#include <cstdlib>

typedef pcl::PointCloud<pcl::PointXYZRGB> PointCloudRGB;
typedef pcl::PointCloud<pcl::Normal> PointCloudNormal;

struct InitialAlignmentReplay
{
    static void cluster(InitialAlignment& ia, PointCloudRGB::Ptr cloud, PointCloudNormal::Ptr normals,
                        std::vector<pcl::PointIndices>& out)
    {
        ia.obtainNormalsCluster(cloud, normals, out);
    }
    static void dominant(InitialAlignment& ia, PointCloudNormal::Ptr normals, const std::vector<pcl::PointIndices>& c,
                         PointCloudNormal::Ptr out)
    {
        ia.obtainDominantNormals(normals, c, out);
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

template <class T>
static bool write_all(const char* path, const std::vector<T>& v)
{
    FILE* f = std::fopen(path, "wb");
    if (!f)
        return false;
    if (!v.empty())
        std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 6)
    {
        std::fprintf(stderr, "usage: %s cloud.bin normals.bin indices.bin sizes.bin dominant.bin\n", argv[0]);
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

    // normals that do not match the cloud: no cluster is found, the fallback of one cluster 0 .. n - 1
    {
        PointCloudNormal::Ptr fewer(new PointCloudNormal(*normals));
        if (!fewer->points.empty())
            fewer->points.pop_back();
        std::vector<pcl::PointIndices> fb;
        InitialAlignmentReplay::cluster(ia, cloud, fewer, fb);
        bool whole = fb.size() == 1 && fb[0].indices.size() == cloud->points.size();
        for (std::size_t i = 0; whole && i < fb[0].indices.size(); ++i)
            whole = fb[0].indices[i] == static_cast<int>(i);
        check(whole, "size_mismatch_falls_back_to_one_cluster");
        check(ros::error_count() == 1, "the_fallback_is_logged");
    }
    const int errors_before = ros::error_count();

    std::vector<pcl::PointIndices> clusters;
    InitialAlignmentReplay::cluster(ia, cloud, normals, clusters);
    std::vector<int> indices, sizes;
    bool ascending = true, seeds_ascend = true;
    for (std::size_t c = 0; c < clusters.size(); ++c)
    {
        const std::vector<int>& m = clusters[c].indices;
        for (std::size_t i = 1; i < m.size(); ++i)
            ascending = ascending && m[i - 1] < m[i];
        seeds_ascend = seeds_ascend && !m.empty() && (c == 0 || clusters[c - 1].indices[0] < m[0]);
        indices.insert(indices.end(), m.begin(), m.end());
        sizes.push_back(static_cast<int>(m.size()));
    }
    check(!clusters.empty(), "clusters_found");
    check(ascending, "members_ascend");
    check(seeds_ascend, "clusters_come_in_ascending_seed");

    PointCloudNormal::Ptr dominant(new PointCloudNormal);
    pcl::Normal old;
    old.normal_x = 7.f;
    dominant->points.push_back(old);  // the reference appends
    InitialAlignmentReplay::dominant(ia, normals, clusters, dominant);
    check(dominant->points.size() == 1 + clusters.size() && dominant->points[0].normal_x == 7.f,
          "dominant_normals_are_appended");
    std::vector<float> dom;
    for (std::size_t c = 1; c < dominant->points.size(); ++c)
    {
        dom.push_back(dominant->points[c].normal_x);
        dom.push_back(dominant->points[c].normal_y);
        dom.push_back(dominant->points[c].normal_z);
    }
    std::printf("clusters %zu clustered %zu\n", clusters.size(), indices.size());
    if (!write_all(argv[3], indices) || !write_all(argv[4], sizes) || !write_all(argv[5], dom))
    {
        std::fprintf(stderr, "cannot write the outputs\n");
        return 2;
    }
    check(ros::error_count() == errors_before, "no_error_logged");
    return g_fail ? 1 : 0;
}
