/*
 * adapter/InitialAlignment_correspondences_mi355x.cpp -- InitialAlignment::obtainCorrespondences over the
 * MI355X engine.
 * Replaces the body of
 *     InitialAlignment::obtainCorrespondences   (src/InitialAlignment.cpp:510-517 of the reference:
 *                          pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33>
 *                          ::determineCorrespondences from source_features_ to target_features_, its
 *                          max_distance left at the default; every keypoint method calls it)
 * Delete that definition from src/InitialAlignment.cpp and add this file to the library sources
 * (INTEGRATION.md section 2); the other members keep their reference implementations.
 * Compiled inside the catkin workspace.
 */
#include <InitialAlignment.h>

#include <mi355x_gicp.h>

#include <cfloat>
#include <cstddef>
#include <mutex>
#include <vector>

namespace
{
static_assert(sizeof(pcl::FPFHSignature33) == 132, "FPFHSignature33 record must be 33 floats");

// one engine context per process for this member; a context serves one caller at a time
// (include/mi355x_gicp.h "Threading"), so every use takes the mutex
std::mutex& correspondencesMutex()
{
    static std::mutex m;
    return m;
}

mgicp_ctx* correspondencesContext()
{
    static mgicp_ctx* ctx = []() {
        mgicp_ctx* c = nullptr;
        if (mgicp_create(&c, nullptr) != MGICP_OK)
        {
            ROS_ERROR("MI355X engine unavailable: no HIP device?");
            return static_cast<mgicp_ctx*>(nullptr);
        }
        return c;
    }();
    return ctx;
}
}  // namespace

void InitialAlignment::obtainCorrespondences()
{
    const size_t ns = source_features_->points.size();
    const size_t nt = target_features_->points.size();
    // determineCorrespondences replaces whatever the vector held
    correspondences_->clear();
    if (ns != 0 && nt != 0)
    {
        std::lock_guard<std::mutex> lock(correspondencesMutex());
        mgicp_ctx* ctx = correspondencesContext();
        if (!ctx)
            return;
        std::vector<int> match(ns);
        std::vector<float> distance(ns);
        size_t found = 0;
        int rc = mgicp_match_features(ctx, source_features_->points[0].histogram, ns, sizeof(pcl::FPFHSignature33),
                                      target_features_->points[0].histogram, nt, sizeof(pcl::FPFHSignature33),
                                      DBL_MAX, match.data(), distance.data(), &found, nullptr);
        if (rc != MGICP_OK)
        {
            ROS_ERROR("correspondence estimation failed (%d): %s", rc, mgicp_last_error(ctx));
            return;
        }
        // PCL's output: one entry per source feature that found a target, in ascending source index.
        // pcl::Correspondence has a virtual destructor: filled field by field
        correspondences_->resize(found);
        size_t k = 0;
        for (size_t i = 0; i < ns && k < found; ++i)
        {
            if (match[i] < 0)
                continue;
            pcl::Correspondence& c = (*correspondences_)[k++];
            c.index_query = static_cast<int>(i);
            c.index_match = match[i];
            c.distance = distance[i];
        }
    }
    ROS_INFO("Found %zd correspondences", correspondences_->size());
}
