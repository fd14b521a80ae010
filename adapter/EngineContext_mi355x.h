/*
 * adapter/EngineContext_mi355x.h -- the engine context of the stateless helpers: Filter_mi355x.cpp,
 * FODDetector_mi355x.cpp, Utils_mi355x.cpp and InitialAlignment_mi355x.cpp share it.  (GICPAlignment keeps
 * a context of its own: that one has parameters and state.)
 * Inline functions with function-local statics: one context and one mutex per linked library, whatever
 * the number of adapter files in it.  The context is created on first use with default parameters
 * (mgicp_create resolves every kernel).  It holds mutable scratch and one stream and serves one caller at
 * a time (include/mi355x_gicp.h "Threading"): every use takes helperMutex(), so concurrent ROS callbacks
 * (a multi-threaded spinner) serialise on it instead of racing.
 * Include it after a header that brings the ROS log macros (every adapter file's own class header does).
 */
#pragma once

#include <mi355x_gicp.h>

#include <mutex>

namespace mi355x
{
inline std::mutex& helperMutex()
{
    static std::mutex m;
    return m;
}

// null when no engine can be created: logged once, the callers return their failure value
inline mgicp_ctx* helperContext()
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
}  // namespace mi355x
