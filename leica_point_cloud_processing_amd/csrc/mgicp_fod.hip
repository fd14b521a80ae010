// mgicp_fod.hip -- the product calls beside the alignment (include/mi355x_gicp.h): point transforms,
// cloud resolution, the radius filter, radius normals, boundary points, Harris keypoints, FPFH descriptors, feature
// correspondences, segment differences, Euclidean clustering and the voxel grid.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "host_upload.hpp"
#include "mgicp_ctx.hpp"

using namespace mgicp;

namespace {

// Euclidean clustering's same-cell shortcut: on a grid of edge h = tol / 2 with at most this many cells
// per axis, any two points of one cell are linked (float d2 < float(tol^2)), so they are united
// without a distance test.  With u = 2^-24 and H = 1 / inv_h <= h (1 + u): two points of cell c on an
// axis have fl(fl(v - o) inv_h) in [c, c + 1), so their a = fl(v - o) differ by less than
// H (1 + 2 (c + 1) u), and v - o = a (1 +- u) with a <= ext; as c H <= ext (1 + 2 u) and
// ext <= N H for N cells, |v1 - v2| < H (1 + 4 u N + 4 u) <= h (1 + 2^-4 + 2^-21) at N <= 2^18, i.e.
// < 0.5313 tol.  Exact d^2 < 3 * 0.5313^2 tol^2 < 0.847 tol^2; FLANN's float expression (a rounded
// difference, three rounded squares, two rounded sums) exceeds the exact value by less than a factor
// 1 + 2^-21, and float(tol^2) >= tol^2 (1 - u) while it is a normal float: 0.847 (1 + 2^-21) < 1 - u.
// A grid grown past tol / 2 (kMaxCells), wider than 2^18 cells or with a denormal / infinite
// float(tol^2) takes the path that tests the pairs inside a cell too.
constexpr int kCcShortcutMaxDim = 1 << 18;

// a function-local device buffer, released on every exit.  (DevBuf itself has no destructor: the target
// cache's buffers are globals and would call hipFree at process exit.)
template <class T>
struct ScopedBuf : DevBuf<T> {
  ~ScopedBuf() { this->release(); }
};

// the transform of n packed device points, their x, y, z scattered into strided host records
int xform_to_host(mgicp_ctx* ctx, const float4* d_in, size_t n, const float T_cm[16], float* out, size_t out_stride) {
  ScopedBuf<float4> d_xf;
  HIPCK(d_xf.reserve(n));
  HIPCK(launch_xform_points(d_in, n, Mat4::from_cm(T_cm).xf(), d_xf.p, ctx->stream));
  std::vector<float4> h(n);
  HIPCK(hipMemcpyAsync(h.data(), d_xf.p, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  int rc = sync(ctx);
  if (rc) return rc;
  unsigned char* base = reinterpret_cast<unsigned char*>(out);
  for (size_t i = 0; i < n; ++i) {
    float* o = reinterpret_cast<float*>(base + i * out_stride);
    o[0] = h[i].x;
    o[1] = h[i].y;
    o[2] = h[i].z;
  }
  return MGICP_OK;
}

// Upload a cloud into ctx->aux and build its grid over the finite points (the reference's KdTreeFLANN
// holds only those); force_h > 0: with that cell edge.  Both flags are the call's own and are back at
// their defaults on every return.  An empty grid (no finite point) is not an error: callers check aux.n.
int aux_grid(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, double force_h = 0.0) {
  int rc = upload_cloud(ctx, ctx->aux, xyz, n, stride, false);
  if (rc) return rc;
  ctx->aux.drop_nonfinite = true;
  ctx->aux.force_h = force_h;
  rc = build_grid(ctx, ctx->aux);
  ctx->aux.drop_nonfinite = false;
  ctx->aux.force_h = 0.0;
  return rc;
}

}  // namespace

extern "C" {

int mgicp_transform_source(mgicp_ctx* ctx, const float T_cm[16], float* out, size_t out_stride) {
  if (!ctx || !T_cm || !out || out_stride < 12 || (out_stride % 4) || ctx->src.n == 0) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  return xform_to_host(ctx, ctx->src.orig.p, ctx->src.n, T_cm, out, out_stride);
}

int mgicp_transform_cloud(mgicp_ctx* ctx, const float T_cm[16], const float* in, size_t n,
                          size_t in_stride, float* out, size_t out_stride) {
  if (!ctx || !T_cm || (n && (!in || !out)) || in_stride < 12 || out_stride < 12 ||
      (in_stride % 4) || (out_stride % 4))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  if (n == 0) return MGICP_OK;
  ScopedBuf<unsigned char> raw;
  ScopedBuf<float4> packed;
  HIPCK(raw.reserve(n * in_stride));
  HIPCK(packed.reserve(n));
  HIPCK(hipMemcpyAsync(raw.p, in, n * in_stride, hipMemcpyHostToDevice, ctx->stream));
  HIPCK(launch_pack_points(raw.p, n, in_stride, packed.p, ctx->stream));
  return xform_to_host(ctx, packed.p, n, T_cm, out, out_stride);
}

int mgicp_cloud_resolution(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, double* out) {
  if (!ctx || !out) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  *out = 0.0;
  if (n < 2) return MGICP_OK;  // no point has a 2nd neighbour: res stays 0
  // Utils::computeCloudResolution skips non-finite points and its KdTree holds only finite ones
  // (src/Utils.cpp:152-160): grid and queries over the finite points
  int rc = aux_grid(ctx, xyz, n, stride);
  if (rc) return rc;
  const size_t nf = ctx->aux.n;
  if (nf < 2) return MGICP_OK;  // nearestKSearch never returns 2: n_points = 0, res = 0
  const int nb = static_cast<int>((nf + 255) / 256);
  HIPCK(ctx->partial.reserve(static_cast<size_t>(nb) * kRedVals));
  HIPCK(ctx->red.reserve(kRedVals));
  if ((rc = ensure_host_red(ctx))) return rc;
  HIPCK(launch_resolution(ctx->aux.view, nf, ctx->partial.p, nb, ctx->stream));
  HIPCK(launch_reduce_finish(ctx->partial.p, nb, ctx->red.p, ctx->stream));
  HIPCK(hipMemcpyAsync(ctx->h_red, ctx->red.p, kRedVals * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = sync(ctx))) return rc;
  const double cnt = ctx->h_red[13];
  *out = cnt > 0 ? ctx->h_red[0] / cnt : 0.0;
  return MGICP_OK;
}

int mgicp_radius_filter(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, double radius,
                        int min_neighbors, unsigned char* keep) {
  if (!ctx || !keep || min_neighbors < 1 || !(radius >= 0)) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  if (n == 0) return MGICP_OK;
  // NormalEstimation gives non-finite points NaN normals and searches a tree of the finite points
  // only: grid over the finite points, keep = 0 for every other record
  int rc = aux_grid(ctx, xyz, n, stride);
  if (rc) return rc;
  ScopedBuf<unsigned char> d_keep;
  HIPCK(d_keep.reserve(n));
  HIPCK(hipMemsetAsync(d_keep.p, 0, n, ctx->stream));
  const float r2 = static_cast<float>(radius * radius);
  // one query per finite point; the kernel scatters keep[] through the original index in w
  HIPCK(launch_radius_keep(ctx->aux.view, ctx->aux.n, r2, min_neighbors, d_keep.p, ctx->stream));
  HIPCK(hipMemcpyAsync(keep, d_keep.p, n, hipMemcpyDeviceToHost, ctx->stream));
  return sync(ctx);
}

int mgicp_estimate_normals(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, double radius,
                           const float viewpoint[3], float* normals, size_t normal_stride, float* curvature,
                           int* n_neighbors, mgicp_normals_info* info) {
  if (!ctx || !(radius >= 0) || (n && (!xyz || !normals)) || stride < 12 || (stride % 4) || normal_stride < 12 ||
      (normal_stride % 4))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_normals_info inf{};
  if (info) *info = inf;
  if (n == 0) return MGICP_OK;
  // FLANN's radius: float(radius^2), strict.  0 links nothing, not even a point with itself
  const float r2 = static_cast<float>(radius * radius);
  // every neighbour lies within `reach` per axis; a denormal r2 may be far above radius^2
  double reach = radius;
  if (r2 < 1.17549435e-38f) reach = std::max(reach, std::sqrt(static_cast<double>(r2)));
  // the tree holds the finite records only: grid over those, at a cell edge of one radius (a query's
  // neighbours then lie in a block of about 3 x 3 x 3 cells; the kernel is exact for any edge)
  int rc = aux_grid(ctx, xyz, n, stride, r2 > 0.f ? std::min(reach, 1e30) : 0.0);
  if (rc) return rc;
  const double t1 = now_ms();
  const size_t nf = ctx->aux.n;
  hipStream_t s = ctx->stream;
  ScopedBuf<float4> d_out;
  ScopedBuf<int> d_cnt;
  HIPCK(d_out.reserve(n));
  HIPCK(d_cnt.reserve(n));
  HIPCK(ctx->cc_tests.reserve(1));
  const float vp[3] = {viewpoint ? viewpoint[0] : 0.f, viewpoint ? viewpoint[1] : 0.f, viewpoint ? viewpoint[2] : 0.f};
  const double t2 = now_ms();
  // records outside the grid (non-finite) keep these: a quiet NaN in every component, no neighbour
  HIPCK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_out.p), 0x7fc00000, n * 4, s));
  HIPCK(hipMemsetAsync(d_cnt.p, 0, n * sizeof(int), s));
  HIPCK(hipMemsetAsync(ctx->cc_tests.p, 0, sizeof(unsigned long long), s));
  HIPCK(launch_normals_tile(ctx->aux.view, nf, r2, vp, d_out.p, d_cnt.p, ctx->cc_tests.p, s));
  if ((rc = sync(ctx))) return rc;
  const double t3 = now_ms();
  std::vector<float4> ho(n);
  std::vector<int> hc(n_neighbors ? 0 : n);
  int* cnt = n_neighbors ? n_neighbors : hc.data();
  unsigned long long ntests = 0;
  HIPCK(hipMemcpyAsync(ho.data(), d_out.p, n * sizeof(float4), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(cnt, d_cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&ntests, ctx->cc_tests.p, sizeof(ntests), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  unsigned char* base = reinterpret_cast<unsigned char*>(normals);
  size_t n_nan = 0;
  for (size_t i = 0; i < n; ++i) {
    float* o = reinterpret_cast<float*>(base + i * normal_stride);
    o[0] = ho[i].x;
    o[1] = ho[i].y;
    o[2] = ho[i].z;
    if (curvature) curvature[i] = ho[i].w;
    n_nan += !(ho[i].x == ho[i].x && ho[i].y == ho[i].y && ho[i].z == ho[i].z);
  }
  inf.n_finite = static_cast<double>(nf);
  inf.n_nan = static_cast<double>(n_nan);
  inf.pair_tests = static_cast<double>(ntests);
  inf.ms_grid = t1 - t0;
  inf.ms_device = t3 - t2;
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_boundary_points(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, const float* normals,
                          size_t normal_stride, int k, double angle_threshold, unsigned char* boundary, float* max_gap,
                          int* nn_indices, mgicp_boundary_info* info) {
  if (!ctx || k < 1 || k > kMaxK || angle_threshold != angle_threshold || (n && (!xyz || !normals || !boundary)) ||
      stride < 12 || (stride % 4) || normal_stride < 12 || (normal_stride % 4))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_boundary_info inf{};
  if (info) *info = inf;
  if (n == 0) return MGICP_OK;
  // the tree holds the finite records only; the grid is sized by occupancy like a set cloud's
  int rc = aux_grid(ctx, xyz, n, stride);
  if (rc) return rc;
  const size_t nf = ctx->aux.n;
  hipStream_t s = ctx->stream;
  const size_t nk = n * static_cast<size_t>(k);
  std::vector<float> hn(3 * n);
  const unsigned char* nbase = reinterpret_cast<const unsigned char*>(normals);
  for (size_t i = 0; i < n; ++i) std::memcpy(&hn[3 * i], nbase + i * normal_stride, 12);
  ScopedBuf<float> d_nrm, d_gap;
  ScopedBuf<unsigned char> d_flag;
  ScopedBuf<int> d_nn;
  ScopedBuf<uint32_t> d_fb;
  ScopedBuf<unsigned int> d_cnt;
  HIPCK(d_nrm.reserve(3 * n));
  HIPCK(d_gap.reserve(n));
  HIPCK(d_flag.reserve(n));
  HIPCK(d_fb.reserve(std::max<size_t>(nf, 1)));
  HIPCK(d_cnt.reserve(1));
  if (nn_indices) HIPCK(d_nn.reserve(nk));
  HIPCK(ctx->cc_tests.reserve(1));
  HIPCK(hipMemcpyAsync(d_nrm.p, hn.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  // records that are never boundary points keep these: flag 0, gap a quiet NaN, every index -1
  HIPCK(hipMemsetAsync(d_flag.p, 0, n, s));
  HIPCK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_gap.p), 0x7fc00000, n, s));
  if (nn_indices) HIPCK(hipMemsetAsync(d_nn.p, 0xff, nk * sizeof(int), s));
  HIPCK(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned int), s));
  HIPCK(hipMemsetAsync(ctx->cc_tests.p, 0, sizeof(unsigned long long), s));
  HIPCK(launch_boundary(ctx->aux.view, nf, d_nrm.p, k, static_cast<float>(angle_threshold), d_flag.p, d_gap.p,
                        nn_indices ? d_nn.p : nullptr, d_fb.p, d_cnt.p, ctx->cc_tests.p, s));
  if ((rc = sync(ctx))) return rc;
  const double t2 = now_ms();
  std::vector<float> hg(max_gap ? 0 : n);
  float* gp = max_gap ? max_gap : hg.data();
  unsigned long long ntests = 0;
  HIPCK(hipMemcpyAsync(boundary, d_flag.p, n, hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(gp, d_gap.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (nn_indices) HIPCK(hipMemcpyAsync(nn_indices, d_nn.p, nk * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&ntests, ctx->cc_tests.p, sizeof(ntests), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  size_t n_boundary = 0, n_nan = 0;
  for (size_t i = 0; i < n; ++i) {
    n_boundary += boundary[i] != 0;
    n_nan += gp[i] != gp[i];
  }
  inf.n_finite = static_cast<double>(nf);
  inf.n_boundary = static_cast<double>(n_boundary);
  inf.n_undecided = static_cast<double>(n_nan - (n - nf));  // every non-finite record has a NaN gap
  inf.pair_tests = static_cast<double>(ntests);
  inf.ms_grid = t1 - t0;
  inf.ms_device = t2 - t1;
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_harris_keypoints(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, const float* normals,
                           size_t normal_stride, double radius, float threshold, int nonmax, int* keypoints,
                           size_t* n_keypoints, float* response, float* covar, int* n_neighbors,
                           mgicp_harris_info* info) {
  if (!ctx || !(radius >= 0) || threshold != threshold || !n_keypoints || (n && (!xyz || !normals || !keypoints)) ||
      stride < 12 || (stride % 4) || normal_stride < 12 || (normal_stride % 4) || n > size_t(INT32_MAX))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_harris_info inf{};
  if (info) *info = inf;
  *n_keypoints = 0;
  if (n == 0) return MGICP_OK;
  // FLANN's radius: float(radius^2), strict.  0 links nothing, not even a point with itself
  const float r2 = static_cast<float>(radius * radius);
  double reach = radius;
  if (r2 < 1.17549435e-38f) reach = std::max(reach, std::sqrt(static_cast<double>(r2)));
  // the tree holds the finite records only: grid over those, at a cell edge of one radius
  int rc = aux_grid(ctx, xyz, n, stride, r2 > 0.f ? std::min(reach, 1e30) : 0.0);
  if (rc) return rc;
  const size_t nf = ctx->aux.n;
  hipStream_t s = ctx->stream;
  std::vector<float> hn(3 * n);
  const unsigned char* nbase = reinterpret_cast<const unsigned char*>(normals);
  for (size_t i = 0; i < n; ++i) std::memcpy(&hn[3 * i], nbase + i * normal_stride, 12);
  ScopedBuf<float> d_nrm, d_rpos, d_resp, d_cov;
  ScopedBuf<float4> d_pack;
  ScopedBuf<int> d_cnt;
  ScopedBuf<uint32_t> d_flag, d_pos, d_list, d_fb;
  ScopedBuf<unsigned char> d_scratch;
  ScopedBuf<unsigned int> d_fbn;
  ScopedBuf<unsigned long long> d_ctr;
  const size_t sb = scan_scratch_bytes(n + 1);
  HIPCK(d_nrm.reserve(3 * n));
  HIPCK(d_pack.reserve(std::max<size_t>(nf, 1)));
  HIPCK(d_rpos.reserve(std::max<size_t>(nf, 1)));
  HIPCK(d_fb.reserve(std::max<size_t>(nf, 1)));
  if (response) HIPCK(d_resp.reserve(n));
  if (covar) HIPCK(d_cov.reserve(6 * n));
  if (n_neighbors) HIPCK(d_cnt.reserve(n));
  HIPCK(d_flag.reserve(n + 1));
  HIPCK(d_pos.reserve(n + 1));
  HIPCK(d_list.reserve(n));
  HIPCK(d_scratch.reserve(sb));
  HIPCK(d_fbn.reserve(1));
  HIPCK(d_ctr.reserve(3 * kHarCtrSlots));
  HIPCK(hipMemcpyAsync(d_nrm.p, hn.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  // records outside the grid (non-finite) keep these: response 0, covar 0, no neighbour, no flag; list
  // entries past the count stay -1
  if (response) HIPCK(hipMemsetAsync(d_resp.p, 0, n * sizeof(float), s));
  if (covar) HIPCK(hipMemsetAsync(d_cov.p, 0, 6 * n * sizeof(float), s));
  if (n_neighbors) HIPCK(hipMemsetAsync(d_cnt.p, 0, n * sizeof(int), s));
  HIPCK(hipMemsetAsync(d_flag.p, 0, (n + 1) * sizeof(uint32_t), s));
  HIPCK(hipMemsetAsync(d_list.p, 0xff, n * sizeof(uint32_t), s));
  HIPCK(hipMemsetAsync(d_ctr.p, 0, 3 * kHarCtrSlots * sizeof(unsigned long long), s));
  const GridView& g = ctx->aux.view;
  // 1. normals to grid order, moments and response; 2. suppression over the candidates; 3. the flagged
  // records listed in ascending original index
  HIPCK(launch_harris_response(g, nf, d_nrm.p, d_pack.p, r2, threshold, d_rpos.p, response ? d_resp.p : nullptr,
                               covar ? d_cov.p : nullptr, n_neighbors ? d_cnt.p : nullptr, d_fb.p, d_fbn.p, d_ctr.p, s));
  if (nonmax) {
    HIPCK(launch_harris_nms(g, nf, d_rpos.p, r2, threshold, d_flag.p, d_fb.p, d_fbn.p, d_ctr.p, s));
    HIPCK(launch_harris_compact(d_flag.p, d_pos.p, n, d_scratch.p, sb, d_list.p, s));
  }
  if ((rc = sync(ctx))) return rc;
  const double t2 = now_ms();
  unsigned long long slots[3 * kHarCtrSlots], ctr[3] = {0, 0, 0};
  uint32_t nkp = 0;
  if (nonmax) {
    HIPCK(hipMemcpyAsync(keypoints, d_list.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCK(hipMemcpyAsync(&nkp, d_pos.p + n, sizeof(nkp), hipMemcpyDeviceToHost, s));
  }
  if (response) HIPCK(hipMemcpyAsync(response, d_resp.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (covar) HIPCK(hipMemcpyAsync(covar, d_cov.p, 6 * n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (n_neighbors) HIPCK(hipMemcpyAsync(n_neighbors, d_cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(slots, d_ctr.p, sizeof(slots), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  for (int i = 0; i < 3 * kHarCtrSlots; ++i) ctr[i % 3] += slots[i];
  if (!nonmax) {  // PCL's branch: the whole response cloud, every record
    for (size_t i = 0; i < n; ++i) keypoints[i] = static_cast<int>(i);
    nkp = static_cast<uint32_t>(n);
  }
  *n_keypoints = nkp;
  inf.n_finite = static_cast<double>(nf);
  inf.n_candidates = static_cast<double>(ctr[1]);
  inf.n_keypoints = static_cast<double>(nkp);
  inf.n_tied = static_cast<double>(ctr[2]);
  inf.pair_tests = static_cast<double>(ctr[0]);
  inf.ms_grid = t1 - t0;
  inf.ms_device = t2 - t1;
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_fpfh_features(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, const float* normals,
                        size_t normal_stride, const int* keypoints, size_t n_keypoints, double radius, float* fpfh,
                        size_t fpfh_stride, uint16_t* spfh_counts, int* spfh_sizes, mgicp_fpfh_info* info) {
  const size_t nk = keypoints ? n_keypoints : n;
  if (!ctx || !(radius >= 0) || (n && (!xyz || !normals)) || (nk && !fpfh) || stride < 12 || (stride % 4) ||
      normal_stride < 12 || (normal_stride % 4) || fpfh_stride < 132 || (fpfh_stride % 4) || n > size_t(INT32_MAX))
    return MGICP_E_INVALID;
  for (size_t k = 0; keypoints && k < nk; ++k)
    if (keypoints[k] < 0 || static_cast<size_t>(keypoints[k]) >= n)
      return fail(ctx, MGICP_E_INVALID, "keypoint index outside [0, n)");
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_fpfh_info inf{};
  if (info) *info = inf;
  if (spfh_counts && n) std::memset(spfh_counts, 0, n * 33 * sizeof(uint16_t));
  if (spfh_sizes && n) std::memset(spfh_sizes, 0, n * sizeof(int));
  if (n == 0 || nk == 0) return MGICP_OK;
  // FLANN's radius: float(radius^2), strict.  0 links nothing, not even a point with itself
  const float r2 = static_cast<float>(radius * radius);
  double reach = radius;
  if (r2 < 1.17549435e-38f) reach = std::max(reach, std::sqrt(static_cast<double>(r2)));
  // the tree holds the finite records only: grid over those, at a cell edge of one radius
  int rc = aux_grid(ctx, xyz, n, stride, r2 > 0.f ? std::min(reach, 1e30) : 0.0);
  if (rc) return rc;
  const size_t nf = ctx->aux.n;
  hipStream_t s = ctx->stream;
  unsigned char* obase = reinterpret_cast<unsigned char*>(fpfh);
  if (nf == 0) {  // no finite record: every keypoint's is non-finite
    for (size_t k = 0; k < nk; ++k) {
      float* o = reinterpret_cast<float*>(obase + k * fpfh_stride);
      for (int b = 0; b < 33; ++b) o[b] = std::nanf("");
    }
    inf.n_keypoints = inf.n_nan = static_cast<double>(nk);
    inf.ms_grid = inf.ms_total = now_ms() - t0;
    if (info) *info = inf;
    return MGICP_OK;
  }
  std::vector<float> hn(3 * n);
  const unsigned char* nbase = reinterpret_cast<const unsigned char*>(normals);
  for (size_t i = 0; i < n; ++i) std::memcpy(&hn[3 * i], nbase + i * normal_stride, 12);
  ScopedBuf<float> d_nrm, d_out;
  ScopedBuf<int> d_kp, d_msize;
  ScopedBuf<uint32_t> d_posof, d_mark, d_pos, d_list;
  ScopedBuf<uint16_t> d_rows;
  ScopedBuf<unsigned char> d_scratch;
  ScopedBuf<unsigned int> d_big;
  ScopedBuf<unsigned long long> d_ctr;
  const size_t sb = scan_scratch_bytes(nf + 1);
  HIPCK(d_nrm.reserve(3 * n));
  HIPCK(d_out.reserve(nk * 33));
  if (keypoints) HIPCK(d_kp.reserve(nk));
  HIPCK(d_msize.reserve(nf));
  HIPCK(d_posof.reserve(n));
  HIPCK(d_mark.reserve(nf + 1));
  HIPCK(d_pos.reserve(nf + 1));
  HIPCK(d_list.reserve(nf));
  HIPCK(d_rows.reserve(nf * 33));
  HIPCK(d_scratch.reserve(sb));
  HIPCK(d_big.reserve(1));
  HIPCK(d_ctr.reserve(2 * kFpfhCtrSlots));
  HIPCK(hipMemcpyAsync(d_nrm.p, hn.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  if (keypoints) HIPCK(hipMemcpyAsync(d_kp.p, keypoints, nk * sizeof(int), hipMemcpyHostToDevice, s));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  // records outside the union keep a zero row and size; records outside the grid have no position
  HIPCK(hipMemsetAsync(d_posof.p, 0xff, n * sizeof(uint32_t), s));
  HIPCK(hipMemsetAsync(d_rows.p, 0, nf * 33 * sizeof(uint16_t), s));
  HIPCK(hipMemsetAsync(d_msize.p, 0, nf * sizeof(int), s));
  HIPCK(hipMemsetAsync(d_big.p, 0, sizeof(unsigned int), s));
  HIPCK(hipMemsetAsync(d_ctr.p, 0, 2 * kFpfhCtrSlots * sizeof(unsigned long long), s));
  const GridView& g = ctx->aux.view;
  const int* kp = keypoints ? d_kp.p : nullptr;
  // 1. the union of the keypoints' sets, listed; 2. its SPFH rows; 3. the keypoints' histograms
  HIPCK(launch_fpfh_mark(g, nf, kp, nk, r2, d_posof.p, d_mark.p, d_pos.p, d_list.p, d_scratch.p, sb, d_big.p, d_ctr.p, s));
  HIPCK(launch_fpfh_spfh(g, nf, d_list.p, d_pos.p + nf, d_nrm.p, r2, d_rows.p, d_msize.p, d_big.p, d_ctr.p, s));
  HIPCK(launch_fpfh_final(g, kp, nk, d_posof.p, r2, d_rows.p, d_msize.p, d_big.p, d_out.p, d_ctr.p, s));
  if ((rc = sync(ctx))) return rc;
  const double t2 = now_ms();
  std::vector<float> ho(nk * 33);
  unsigned long long slots[2 * kFpfhCtrSlots], ctr[2] = {0, 0};
  unsigned int too_big = 0;
  uint32_t n_rows = 0;
  HIPCK(hipMemcpyAsync(ho.data(), d_out.p, nk * 33 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(slots, d_ctr.p, sizeof(slots), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&too_big, d_big.p, sizeof(too_big), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&n_rows, d_pos.p + nf, sizeof(n_rows), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  for (int i = 0; i < 2 * kFpfhCtrSlots; ++i) ctr[i & 1] += slots[i];
  if (too_big) return fail(ctx, MGICP_E_INVALID, "a neighbour set holds more than 65535 records (the limit of an SPFH row)");
  if (spfh_counts || spfh_sizes) {  // rows and sizes come by sorted position: gather through pos_of
    std::vector<uint32_t> pos_of(n);
    std::vector<uint16_t> hr(spfh_counts ? nf * 33 : 0);
    std::vector<int> hm(spfh_sizes ? nf : 0);
    HIPCK(hipMemcpyAsync(pos_of.data(), d_posof.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (spfh_counts) HIPCK(hipMemcpyAsync(hr.data(), d_rows.p, nf * 33 * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
    if (spfh_sizes) HIPCK(hipMemcpyAsync(hm.data(), d_msize.p, nf * sizeof(int), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    for (size_t i = 0; i < n; ++i) {
      const size_t p = pos_of[i];
      if (p >= nf) continue;  // a non-finite record: zero row, size 0
      if (spfh_counts) std::memcpy(spfh_counts + i * 33, &hr[p * 33], 33 * sizeof(uint16_t));
      if (spfh_sizes) spfh_sizes[i] = hm[p];
    }
  }
  // a histogram is NaN exactly when its keypoint's record is not in the grid
  const unsigned char* xbase = reinterpret_cast<const unsigned char*>(xyz);
  size_t n_nan = 0;
  for (size_t k = 0; k < nk; ++k) {
    std::memcpy(obase + k * fpfh_stride, &ho[k * 33], 33 * sizeof(float));
    const float* r = reinterpret_cast<const float*>(xbase + (keypoints ? static_cast<size_t>(keypoints[k]) : k) * stride);
    n_nan += !(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]));
  }
  inf.n_finite = static_cast<double>(nf);
  inf.n_keypoints = static_cast<double>(nk);
  inf.n_nan = static_cast<double>(n_nan);
  inf.n_spfh_rows = static_cast<double>(n_rows);
  inf.pair_tests = static_cast<double>(ctr[0]);
  inf.pair_features = static_cast<double>(ctr[1]);
  inf.ms_grid = t1 - t0;
  inf.ms_device = t2 - t1;
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_match_features(mgicp_ctx* ctx, const float* source, size_t n_source, size_t source_stride,
                         const float* target, size_t n_target, size_t target_stride, double max_distance, int* match,
                         float* distance, size_t* n_correspondences, mgicp_match_info* info) {
  if (!ctx || !(max_distance >= 0) || (n_source && (!source || !match)) || (n_target && !target) ||
      source_stride < 132 || (source_stride % 4) || target_stride < 132 || (target_stride % 4) ||
      n_source > size_t(INT32_MAX) || n_target > size_t(INT32_MAX))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_match_info inf{};
  if (info) *info = inf;
  if (n_correspondences) *n_correspondences = 0;
  std::fill(ctx->match_stats, ctx->match_stats + 8, 0ll);
  const float nanf_ = std::nanf("");
  for (size_t i = 0; i < n_source; ++i) match[i] = -1;
  if (distance) std::fill(distance, distance + n_source, nanf_);
  // the rows with 33 finite values, packed, and the record each came from (ascending: the lowest packed
  // row among equal distances is the lowest record)
  auto pack = [](const float* base, size_t n, size_t stride, std::vector<float>& rows, std::vector<int>& rec) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base);
    rows.reserve(n * 33);
    rec.reserve(n);
    for (size_t i = 0; i < n; ++i) {
      float r[33];
      std::memcpy(r, p + i * stride, sizeof(r));
      bool ok = true;
      for (int b = 0; b < 33; ++b) ok &= std::isfinite(r[b]);
      if (!ok) continue;
      rows.insert(rows.end(), r, r + 33);
      rec.push_back(static_cast<int>(i));
    }
  };
  std::vector<float> hs, ht;
  std::vector<int> srec, trec;
  pack(source, n_source, source_stride, hs, srec);
  pack(target, n_target, target_stride, ht, trec);
  const size_t ns = srec.size(), nt = trec.size();
  inf.n_source_valid = static_cast<double>(ns);
  inf.n_target_valid = static_cast<double>(nt);
  if (ns == 0 || nt == 0) {  // nothing to search with, or nothing to search: every match stays -1
    inf.ms_total = now_ms() - t0;
    if (info) *info = inf;
    return MGICP_OK;
  }
  // target rows of one launch, and the blocks that share them
  const size_t chunk = static_cast<size_t>(
      std::min<unsigned long long>(nt, std::max<unsigned long long>(1, ctx->match_pairs_per_launch / ns)));
  const MatchLayout lay = match_layout(ns, chunk);
  const uint32_t max_splits = std::max(lay.splits, (nt % chunk) ? match_layout(ns, nt % chunk).splits : 1u);
  hipStream_t s = ctx->stream;
  ScopedBuf<float> d_src, d_tgt;
  ScopedBuf<unsigned long long> d_run, d_part, d_ctr;
  std::vector<unsigned long long> keys(ns, kMatchNone);
  HIPCK(d_src.reserve(ns * 33));
  HIPCK(d_tgt.reserve(nt * 33));
  HIPCK(d_run.reserve(ns));
  if (max_splits > 1) HIPCK(d_part.reserve(static_cast<size_t>(max_splits) * ns));
  HIPCK(d_ctr.reserve(3));
  HIPCK(hipMemcpyAsync(d_src.p, hs.data(), ns * 33 * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(d_tgt.p, ht.data(), nt * 33 * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(d_run.p, keys.data(), ns * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  HIPCK(hipMemsetAsync(d_ctr.p, 0, 3 * sizeof(unsigned long long), s));
  int rc = sync(ctx);
  if (rc) return rc;
  const double t1 = now_ms();
  long long launches = 0;
  for (size_t b = 0; b < nt; b += chunk, ++launches)
    HIPCK(launch_match(d_src.p, ns, d_tgt.p, b, std::min(nt, b + chunk), d_run.p, d_part.p, d_ctr.p, s));
  if ((rc = sync(ctx))) return rc;
  const double t2 = now_ms();
  unsigned long long cut[3] = {0, 0, 0};
  HIPCK(hipMemcpyAsync(keys.data(), d_run.p, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(cut, d_ctr.p, sizeof(cut), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  // PCL's rejection, in double: DBL_MAX squares to +inf and rejects nothing
  const double max2 = max_distance * max_distance;
  size_t n_corr = 0, n_tied = 0;
  for (size_t k = 0; k < ns; ++k) {
    const uint32_t low = static_cast<uint32_t>(keys[k]);
    if (low == kMatchNoneLow) continue;
    const uint32_t bits = static_cast<uint32_t>(keys[k] >> 32);
    float d2;
    std::memcpy(&d2, &bits, sizeof(d2));
    if (static_cast<double>(d2) > max2) continue;
    const size_t i = static_cast<size_t>(srec[k]);
    match[i] = trec[low >> 1];
    if (distance) distance[i] = d2;
    ++n_corr;
    n_tied += low & 1u;
  }
  if (n_correspondences) *n_correspondences = n_corr;
  inf.n_correspondences = static_cast<double>(n_corr);
  inf.n_tied = static_cast<double>(n_tied);
  inf.pair_tests = static_cast<double>(ns) * static_cast<double>(nt);  // every pair is begun
  inf.ms_device = t2 - t1;
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  ctx->match_stats[0] = static_cast<long long>(ns) * static_cast<long long>(nt);
  for (int v = 0; v < 3; ++v) ctx->match_stats[1 + v] = static_cast<long long>(cut[v]);
  ctx->match_stats[4] = launches;
  ctx->match_stats[5] = static_cast<long long>(chunk);
  ctx->match_stats[6] = lay.splits;
  ctx->match_stats[7] = lay.per_split;
  return MGICP_OK;
}

int mgicp_segment_differences(mgicp_ctx* ctx, const float T_cm[16], const float* in, size_t n,
                              size_t in_stride, const float* sub, size_t n_sub, size_t sub_stride,
                              double sqr_threshold, unsigned char* keep, size_t* n_keep) {
  if (!ctx || !n_keep || (n && (!in || !keep)) || (n_sub && !sub) || !(sqr_threshold == sqr_threshold))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  *n_keep = 0;
  if (n == 0) return MGICP_OK;
  if (n_sub == 0) {  // "input - empty target = input": every record, finite or not
    std::memset(keep, 1, n);
    *n_keep = n;
    return MGICP_OK;
  }
  int rc = aux_grid(ctx, sub, n_sub, sub_stride);
  if (rc) return rc;
  if (ctx->aux.n == 0) {  // no finite target point: nearestKSearch finds nothing, nothing kept
    std::memset(keep, 0, n);
    return MGICP_OK;
  }
  if ((rc = upload_cloud(ctx, ctx->qry, in, n, in_stride, false))) return rc;
  hipStream_t s = ctx->stream;
  HIPCK(ctx->f_keep.reserve(n));
  HIPCK(ctx->f_count.reserve(1));
  HIPCK(hipMemsetAsync(ctx->f_count.p, 0, sizeof(unsigned int), s));
  const Mat4 T = T_cm ? Mat4::from_cm(T_cm) : Mat4::identity();
  HIPCK(launch_segdiff(ctx->aux.view, ctx->qry.orig.p, n, T.xf(), T_cm ? 1 : 0, sqr_threshold,
                       ctx->f_keep.p, ctx->f_count.p, s));
  HIPCK(hipMemcpyAsync(keep, ctx->f_keep.p, n, hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(ctx->h_small, ctx->f_count.p, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  unsigned int cnt = 0;
  std::memcpy(&cnt, ctx->h_small, sizeof(cnt));
  *n_keep = cnt;
  return MGICP_OK;
}

int mgicp_euclidean_clusters(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, double tolerance,
                             size_t min_size, size_t max_size, int* labels, int* indices, size_t* offsets,
                             mgicp_cluster_info* info) {
  if (!ctx || !(tolerance >= 0) || !offsets || (n && (!xyz || !labels || !indices))) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_cluster_info inf{};
  if (info) *info = inf;
  offsets[0] = 0;
  if (n == 0) return MGICP_OK;
  // FLANN's radius: float(tolerance^2), strict.  0 links nothing (not even duplicates): singletons
  const float r2 = static_cast<float>(tolerance * tolerance);
  const bool link = r2 > 0.f;
  // every linked pair lies within `reach` per axis; a denormal r2 may be far above tolerance^2
  double reach = tolerance;
  if (r2 < 1.17549435e-38f) reach = std::max(reach, std::sqrt(static_cast<double>(r2)));
  // non-finite records join no cluster: grid (and forest) over the finite points, label -1 for the rest
  int rc = aux_grid(ctx, xyz, n, stride, link ? 0.5 * reach : 0.0);
  if (rc) return rc;
  std::fill(labels, labels + n, -1);
  std::fill(offsets, offsets + n + 1, size_t(0));
  const double t1 = now_ms();
  const size_t nf = ctx->aux.n;
  if (nf == 0) return MGICP_OK;
  const GridView& g = ctx->aux.view;
  const bool shortcut = link && r2 >= 1.17549435e-38f && std::isfinite(r2) &&
                        g.inv_h == static_cast<float>(1.0 / (0.5 * tolerance)) &&
                        std::max(g.nx, std::max(g.ny, g.nz)) <= kCcShortcutMaxDim;
  hipStream_t s = ctx->stream;
  int bits = 1;
  while ((size_t(1) << bits) < n && bits < 32) ++bits;
  const size_t sb = sort_scratch_bytes(nf, bits);
  // the context keeps these buffers between calls (like the grid's scratch)
  HIPCK(ctx->cc_parent.reserve(nf));
  HIPCK(ctx->cc_root.reserve(nf));
  HIPCK(ctx->cc_min.reserve(nf));
  HIPCK(ctx->cc_members.reserve(nf));
  HIPCK(ctx->cc_tests.reserve(1));
  HIPCK(ctx->keys.reserve(nf));
  HIPCK(ctx->vals.reserve(nf));
  HIPCK(ctx->scratch.reserve(sb));
  const double t2 = now_ms();
  HIPCK(hipMemsetAsync(ctx->cc_tests.p, 0, sizeof(unsigned long long), s));
  // build_grid left the sorted cell keys of this grid in keys_sorted
  HIPCK(launch_cc_link(g, nf, ctx->keys_sorted.p, r2, shortcut ? 1 : 0, link ? 1 : 0, ctx->cc_parent.p,
                       ctx->cc_tests.p, s));
  HIPCK(launch_cc_labels(g, ctx->aux.perm.p, nf, ctx->cc_parent.p, ctx->cc_root.p, ctx->cc_min.p, ctx->keys.p,
                         ctx->vals.p, s));
  // the stable sort by component key over records laid out in original order: members ascending
  HIPCK(launch_sort_pairs(ctx->scratch.p, sb, ctx->keys.p, ctx->keys_sorted.p, ctx->vals.p, ctx->cc_members.p, nf,
                          bits, s));
  if ((rc = sync(ctx))) return rc;
  const double t3 = now_ms();
  std::vector<uint32_t> hk(nf), hv(nf);
  unsigned long long ntests = 0;
  HIPCK(hipMemcpyAsync(hk.data(), ctx->keys_sorted.p, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(hv.data(), ctx->cc_members.p, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&ntests, ctx->cc_tests.p, sizeof(ntests), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  // host finish over the component table: runs of equal keys, in ascending smallest-member order
  struct Comp { size_t start, size; };
  std::vector<Comp> kept;
  const size_t lo = std::max<size_t>(min_size, 1), hi = max_size ? max_size : SIZE_MAX;
  int ncomp = 0;
  for (size_t i = 0; i < nf;) {
    size_t j = i + 1;
    while (j < nf && hk[j] == hk[i]) ++j;
    ++ncomp;
    if (j - i >= lo && j - i <= hi) kept.push_back({i, j - i});
    i = j;
  }
  // PCL: sort(clusters.rbegin(), clusters.rend(), by size) over clusters in ascending-seed order;
  // documented choice for equal sizes: ascending smallest member
  std::stable_sort(kept.begin(), kept.end(), [](const Comp& a, const Comp& b) { return a.size > b.size; });
  size_t off = 0;
  for (size_t c = 0; c < kept.size(); ++c) {
    offsets[c] = off;
    for (size_t m = 0; m < kept[c].size; ++m) {
      const uint32_t idx = hv[kept[c].start + m];
      indices[off + m] = static_cast<int>(idx);
      labels[idx] = static_cast<int>(c);
    }
    off += kept[c].size;
  }
  for (size_t c = kept.size(); c <= n; ++c) offsets[c] = off;
  inf.n_clusters = static_cast<int>(kept.size());
  inf.n_components = ncomp;
  inf.n_clustered_points = static_cast<double>(off);
  inf.pair_tests = static_cast<double>(ntests);
  inf.ms_grid = t1 - t0;
  inf.ms_device = t3 - t2;
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_voxel_grid(mgicp_ctx* ctx, const float* in, size_t n, size_t stride, int rgb_offset,
                     const double leaf[3], int min_points_per_voxel, float* out, size_t out_stride,
                     size_t* n_out) {
  // a colour word at offset 0, 4 or 8 would lie over x, y or z of every record, read and written
  if (!ctx || !n_out || !leaf || (n && (!in || !out)) || out_stride < 12 || (out_stride % 4) ||
      (rgb_offset >= 0 && (rgb_offset < 12 || static_cast<size_t>(rgb_offset) + 4 > stride ||
                           static_cast<size_t>(rgb_offset) + 4 > out_stride || (rgb_offset % 4))))
    return MGICP_E_INVALID;
  for (int d = 0; d < 3; ++d)
    if (!(leaf[d] > 0)) return fail(ctx, MGICP_E_INVALID, "leaf size must be > 0");
  HIPCK(hipSetDevice(ctx->device));
  *n_out = 0;
  if (n == 0) return MGICP_OK;
  int rc = upload_cloud(ctx, ctx->qry, in, n, stride, false);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const bool rgb = rgb_offset >= 0;
  if (rgb) {  // the packed colour word of every record, through the pinned pipelined upload
    HIPCK(ctx->f_rgba_in.reserve(n));
    HostUploader& up = HostUploader::instance();
    HIPCK(up.init(ctx->host_threads));
    {
      std::lock_guard<std::mutex> lk(up.mu);
      HIPCK(upload_u32_field(*up.pool, up.ring, in, n, stride, static_cast<size_t>(rgb_offset),
                             ctx->f_rgba_in.p, s));
      if ((rc = sync(ctx))) return rc;
    }
  }
  // getMinMax3D over the finite points
  float mn[3], mx[3];
  if ((rc = bbox_to_host(ctx, ctx->qry.orig.p, n, mn, mx))) return rc;
  if (!(mn[0] <= mx[0])) return MGICP_OK;  // no finite point
  float inv[3];
  for (int d = 0; d < 3; ++d) inv[d] = 1.0f / static_cast<float>(leaf[d]);
  int64_t dd[3];
  for (int d = 0; d < 3; ++d) dd[d] = static_cast<int64_t>((mx[d] - mn[d]) * inv[d]) + 1;
  auto put = [&](size_t i, float x, float y, float z, const uint32_t* c) {
    unsigned char* r = reinterpret_cast<unsigned char*>(out) + i * out_stride;
    std::memset(r, 0, out_stride);
    float* f = reinterpret_cast<float*>(r);
    f[0] = x; f[1] = y; f[2] = z;
    if (out_stride >= 16) f[3] = 1.0f;
    if (c) std::memcpy(r + rgb_offset, c, 4);
  };
  if (dd[0] * dd[1] * dd[2] > static_cast<int64_t>(INT32_MAX)) {
    // "Leaf size is too small for the input dataset": output = input
    const unsigned char* base = reinterpret_cast<const unsigned char*>(in);
    for (size_t i = 0; i < n; ++i) {
      const float* p = reinterpret_cast<const float*>(base + i * stride);
      uint32_t c = 0;
      if (rgb) std::memcpy(&c, base + i * stride + rgb_offset, 4);
      put(i, p[0], p[1], p[2], rgb ? &c : nullptr);
    }
    *n_out = n;
    return MGICP_OK;
  }
  int min_b[3], div_b[3];
  for (int d = 0; d < 3; ++d) {
    min_b[d] = static_cast<int>(std::floor(mn[d] * inv[d]));
    div_b[d] = static_cast<int>(std::floor(mx[d] * inv[d])) - min_b[d] + 1;
  }
  Cloud& q = ctx->qry;
  HIPCK(ctx->keys.reserve(n));
  HIPCK(ctx->keys_sorted.reserve(n));
  HIPCK(ctx->vals.reserve(n));
  HIPCK(q.perm.reserve(n));
  HIPCK(ctx->f_flags.reserve(n + 1));
  HIPCK(ctx->f_pos.reserve(n + 1));
  const size_t sb = std::max(sort_scratch_bytes(n, 32), scan_scratch_bytes(n + 1));
  HIPCK(ctx->scratch.reserve(sb));
  HIPCK(launch_voxel_keys(q.orig.p, n, inv, min_b, div_b[0], div_b[0] * div_b[1], ctx->keys.p, s));
  HIPCK(launch_iota(ctx->vals.p, n, s));
  HIPCK(launch_sort_pairs(ctx->scratch.p, sb, ctx->keys.p, ctx->keys_sorted.p, ctx->vals.p, q.perm.p, n, 32, s));
  HIPCK(launch_voxel_heads(ctx->keys_sorted.p, n, ctx->f_flags.p, s));
  HIPCK(launch_exclusive_scan(ctx->scratch.p, sb, ctx->f_flags.p, ctx->f_pos.p, n + 1, s));
  HIPCK(hipMemcpyAsync(ctx->h_small, ctx->f_pos.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  uint32_t nv = 0;
  std::memcpy(&nv, ctx->h_small, sizeof(nv));
  HIPCK(ctx->f_vox.reserve(nv + 1));
  if (rgb) HIPCK(ctx->f_rgba.reserve(nv + 1));
  HIPCK(launch_voxel_centroids(ctx->keys_sorted.p, q.perm.p, ctx->f_flags.p, ctx->f_pos.p, n, q.orig.p,
                               rgb ? ctx->f_rgba_in.p : nullptr, ctx->f_vox.p, rgb ? ctx->f_rgba.p : nullptr, s));
  const float4* vox = ctx->f_vox.p;
  const uint32_t* vrgb = rgb ? ctx->f_rgba.p : nullptr;
  if (min_points_per_voxel > 1) {
    HIPCK(ctx->f_vox2.reserve(nv + 1));
    if (rgb) HIPCK(ctx->f_rgba2.reserve(nv + 1));
    const size_t sb2 = scan_scratch_bytes(nv + 1);
    HIPCK(ctx->scratch.reserve(std::max(sb, sb2)));
    HIPCK(launch_voxel_minpts(ctx->f_vox.p, vrgb, nv, static_cast<uint32_t>(min_points_per_voxel), ctx->f_flags.p,
                              ctx->f_pos.p, ctx->scratch.p, sb2, ctx->f_vox2.p, rgb ? ctx->f_rgba2.p : nullptr, s));
    HIPCK(hipMemcpyAsync(ctx->h_small, ctx->f_pos.p + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    std::memcpy(&nv, ctx->h_small, sizeof(nv));
    vox = ctx->f_vox2.p;
    vrgb = rgb ? ctx->f_rgba2.p : nullptr;
  }
  std::vector<float4> hv(nv);
  std::vector<uint32_t> hc(rgb ? nv : 0);
  if (nv) {
    HIPCK(hipMemcpyAsync(hv.data(), vox, nv * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (rgb) HIPCK(hipMemcpyAsync(hc.data(), vrgb, nv * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  if ((rc = sync(ctx))) return rc;
  for (size_t v = 0; v < nv; ++v) put(v, hv[v].x, hv[v].y, hv[v].z, rgb ? &hc[v] : nullptr);
  *n_out = nv;
  return MGICP_OK;
}

}  // extern "C"
