// mgicp_features.hip -- the feature calls of the initial alignment (include/mi355x_gicp.h): radius normals,
// boundary points, Harris keypoints, FPFH descriptors and feature correspondences, and the pre-alignment
// transform after them: the RANSAC and one-to-one rejectors and the SVD estimate (their host arithmetic is
// prealign.hpp); and the NORMALS method's own steps, normal clustering and the dominant normals.  Host code only: the kernels and their launchers are in mgicp_kernels.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mi355x_gicp_debug.h"
#include "mgicp_ctx.hpp"
#include "prealign.hpp"

using namespace mgicp;

namespace {

// The tree holds the finite records only: grid over those, at a cell edge of one radius (a query's
// neighbours then lie in a block of about 3 x 3 x 3 cells; the kernels are exact for any edge).  A zero
// r2 links nothing: the grid is then sized by occupancy.
int radius_grid(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, const FlannRadius& fr) {
  return aux_grid(ctx, xyz, n, stride, fr.r2 > 0.f ? std::min(fr.reach, 1e30) : 0.0);
}

// a call's normals: the strided host records packed to 3 * n floats, and their device copy.  upload()
// reads `host` until the stream is synchronised.
struct PackedNormals {
  std::vector<float> host;
  ScopedBuf<float> dev;
  PackedNormals(const float* normals, size_t n, size_t stride) : host(3 * n) {
    const unsigned char* base = reinterpret_cast<const unsigned char*>(normals);
    for (size_t i = 0; i < n; ++i) std::memcpy(&host[3 * i], base + i * stride, 12);
  }
  hipError_t reserve() { return dev.reserve(host.size()); }
  hipError_t upload(hipStream_t s) {
    return hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, s);
  }
};

// the slotted counters of a call's kernels (slot_add in mgicp_kernels.hip): Slots groups of W words on
// the device; fetch() copies them back (valid once the stream is synchronised), add_up() sums them by column
template <int W, int Slots>
struct SlotCounters {
  ScopedBuf<unsigned long long> dev;
  unsigned long long slots[W * Slots];
  unsigned long long sum[W] = {};
  hipError_t reserve() { return dev.reserve(W * Slots); }
  hipError_t zero(hipStream_t s) { return hipMemsetAsync(dev.p, 0, sizeof(slots), s); }
  hipError_t fetch(hipStream_t s) { return hipMemcpyAsync(slots, dev.p, sizeof(slots), hipMemcpyDeviceToHost, s); }
  void add_up() {
    for (int i = 0; i < W * Slots; ++i) sum[i % W] += slots[i];
  }
};

// Normal clustering's angle test without acos on the device: the smallest float f with
// acos((double)f) < eps_angle by this host's libm, found by stepping from float(cos(eps_angle)); the device
// tests d >= c_min && d <= 1.  Nothing is compatible at eps_angle <= 0 (+inf); above pi every d in [-1, 1] is.
float normal_cluster_c_min(double eps_angle) {
  if (!(eps_angle > 0)) return std::numeric_limits<float>::infinity();
  if (eps_angle > M_PI) return -1.0f;
  float f = std::min(1.0f, std::max(-1.0f, static_cast<float>(std::cos(eps_angle))));
  while (f > -1.0f && std::acos(static_cast<double>(std::nextafterf(f, -2.0f))) < eps_angle) f = std::nextafterf(f, -2.0f);
  while (f <= 1.0f && !(std::acos(static_cast<double>(f)) < eps_angle)) f = std::nextafterf(f, 2.0f);
  return f;
}

// ---- the pre-alignment transform: the correspondences of two keypoint clouds on the device ----
// what the three calls refuse before any launch (mi355x_gicp.h "the pre-alignment transform")
bool bad_pairs(const float* src, size_t ns, size_t sstride, const float* tgt, size_t nt, size_t tstride, const int* iq,
               const int* im, size_t m) {
  if ((ns && !src) || (nt && !tgt) || (m && (!iq || !im)) || sstride < 12 || (sstride % 4) || tstride < 12 ||
      (tstride % 4) || ns > size_t(INT32_MAX) || nt > size_t(INT32_MAX) || m > size_t(INT32_MAX))
    return true;
  for (size_t i = 0; i < m; ++i)
    if (iq[i] < 0 || static_cast<size_t>(iq[i]) >= ns || im[i] < 0 || static_cast<size_t>(im[i]) >= nt) return true;
  return false;
}

// the packed host copies (the sampler reads them) and the device copies of the clouds and the index arrays
struct PairSet {
  std::vector<float> hs, ht;
  ScopedBuf<float> d_s, d_t;
  ScopedBuf<int> d_iq, d_im;
  PairView view{};
  static void pack(const float* base, size_t n, size_t stride, std::vector<float>& out) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base);
    out.resize(3 * n);
    for (size_t i = 0; i < n; ++i) std::memcpy(&out[3 * i], p + i * stride, 12);
  }
  // the copies read this object's vectors and the caller's arrays: the stream is synchronised before the
  // call returns, on the error path too, so that none of them is still being read when it goes away
  int upload(mgicp_ctx* ctx, const float* src, size_t ns, size_t sstride, const float* tgt, size_t nt, size_t tstride,
             const int* iq, const int* im, size_t m) {
    pack(src, ns, sstride, hs);
    pack(tgt, nt, tstride, ht);
    hipStream_t s = ctx->stream;
    HIPCK(d_s.reserve(3 * ns));
    HIPCK(d_t.reserve(3 * nt));
    HIPCK(d_iq.reserve(m));
    HIPCK(d_im.reserve(m));
    hipError_t e = hipSuccess;
    if (ns) e = hipMemcpyAsync(d_s.p, hs.data(), 3 * ns * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && nt) e = hipMemcpyAsync(d_t.p, ht.data(), 3 * nt * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && m) e = hipMemcpyAsync(d_iq.p, iq, m * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && m) e = hipMemcpyAsync(d_im.p, im, m * sizeof(int), hipMemcpyHostToDevice, s);
    const int rc = sync(ctx);
    HIPCK(e);
    if (rc) return rc;
    view = PairView{d_s.p, d_t.p, d_iq.p, d_im.p};
    return MGICP_OK;
  }
};

// the 15 sums of a set of pairs, on the device and back (one synchronise)
struct MomentBufs {
  ScopedBuf<double> d_partial, d_out;
  hipError_t reserve(size_t m) {
    hipError_t e = d_partial.reserve(static_cast<size_t>(pair_moment_blocks(m)) * kRedVals);
    return e == hipSuccess ? d_out.reserve(kRedVals) : e;
  }
  int run(mgicp_ctx* ctx, const PairView& v, const uint32_t* list, size_t cnt, double sums[15]) {
    double out[kRedVals];
    HIPCK(launch_pair_moments(v, list, cnt, d_partial.p, d_out.p, ctx->stream));
    HIPCK(hipMemcpyAsync(out, d_out.p, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
    int rc = sync(ctx);
    if (rc) return rc;
    std::copy(out, out + 15, sums);
    return MGICP_OK;
  }
};

void identity_cm(float T[16]) {
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.f : 0.f;
}

// rows of a 3 x 4 -> column-major 4 x 4
void rows_to_cm(const float T[12], float cm[16]) {
  identity_cm(cm);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) cm[4 * c + r] = T[4 * r + c];
}

}  // namespace

extern "C" {

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
  const FlannRadius fr(radius);
  const float r2 = fr.r2;
  int rc = radius_grid(ctx, xyz, n, stride, fr);
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
  PackedNormals nrm(normals, n, normal_stride);
  ScopedBuf<float> d_gap;
  ScopedBuf<unsigned char> d_flag;
  ScopedBuf<int> d_nn;
  ScopedBuf<uint32_t> d_fb;
  ScopedBuf<unsigned int> d_cnt;
  HIPCK(nrm.reserve());
  HIPCK(d_gap.reserve(n));
  HIPCK(d_flag.reserve(n));
  HIPCK(d_fb.reserve(std::max<size_t>(nf, 1)));
  HIPCK(d_cnt.reserve(1));
  if (nn_indices) HIPCK(d_nn.reserve(nk));
  HIPCK(ctx->cc_tests.reserve(1));
  HIPCK(nrm.upload(s));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  // records that are never boundary points keep these: flag 0, gap a quiet NaN, every index -1
  HIPCK(hipMemsetAsync(d_flag.p, 0, n, s));
  HIPCK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_gap.p), 0x7fc00000, n, s));
  if (nn_indices) HIPCK(hipMemsetAsync(d_nn.p, 0xff, nk * sizeof(int), s));
  HIPCK(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned int), s));
  HIPCK(hipMemsetAsync(ctx->cc_tests.p, 0, sizeof(unsigned long long), s));
  HIPCK(launch_boundary(ctx->aux.view, nf, nrm.dev.p, k, static_cast<float>(angle_threshold), d_flag.p, d_gap.p,
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
  const FlannRadius fr(radius);
  const float r2 = fr.r2;
  int rc = radius_grid(ctx, xyz, n, stride, fr);
  if (rc) return rc;
  const size_t nf = ctx->aux.n;
  hipStream_t s = ctx->stream;
  PackedNormals nrm(normals, n, normal_stride);
  ScopedBuf<float> d_rpos, d_resp, d_cov;
  ScopedBuf<float4> d_pack;
  ScopedBuf<int> d_cnt;
  ScopedBuf<uint32_t> d_flag, d_pos, d_list, d_fb;
  ScopedBuf<unsigned char> d_scratch;
  ScopedBuf<unsigned int> d_fbn;
  SlotCounters<3, kHarCtrSlots> ctr;
  const size_t sb = scan_scratch_bytes(n + 1);
  HIPCK(nrm.reserve());
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
  HIPCK(ctr.reserve());
  HIPCK(nrm.upload(s));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  // records outside the grid (non-finite) keep these: response 0, covar 0, no neighbour, no flag; list
  // entries past the count stay -1
  if (response) HIPCK(hipMemsetAsync(d_resp.p, 0, n * sizeof(float), s));
  if (covar) HIPCK(hipMemsetAsync(d_cov.p, 0, 6 * n * sizeof(float), s));
  if (n_neighbors) HIPCK(hipMemsetAsync(d_cnt.p, 0, n * sizeof(int), s));
  HIPCK(hipMemsetAsync(d_flag.p, 0, (n + 1) * sizeof(uint32_t), s));
  HIPCK(hipMemsetAsync(d_list.p, 0xff, n * sizeof(uint32_t), s));
  HIPCK(ctr.zero(s));
  const GridView& g = ctx->aux.view;
  // 1. normals to grid order, moments and response; 2. suppression over the candidates; 3. the flagged
  // records listed in ascending original index
  HIPCK(launch_harris_response(g, nf, nrm.dev.p, d_pack.p, r2, threshold, d_rpos.p, response ? d_resp.p : nullptr,
                               covar ? d_cov.p : nullptr, n_neighbors ? d_cnt.p : nullptr, d_fb.p, d_fbn.p, ctr.dev.p, s));
  if (nonmax) {
    HIPCK(launch_harris_nms(g, nf, d_rpos.p, r2, threshold, d_flag.p, d_fb.p, d_fbn.p, ctr.dev.p, s));
    HIPCK(launch_harris_compact(d_flag.p, d_pos.p, n, d_scratch.p, sb, d_list.p, s));
  }
  if ((rc = sync(ctx))) return rc;
  const double t2 = now_ms();
  uint32_t nkp = 0;
  if (nonmax) {
    HIPCK(hipMemcpyAsync(keypoints, d_list.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCK(hipMemcpyAsync(&nkp, d_pos.p + n, sizeof(nkp), hipMemcpyDeviceToHost, s));
  }
  if (response) HIPCK(hipMemcpyAsync(response, d_resp.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (covar) HIPCK(hipMemcpyAsync(covar, d_cov.p, 6 * n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (n_neighbors) HIPCK(hipMemcpyAsync(n_neighbors, d_cnt.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCK(ctr.fetch(s));
  if ((rc = sync(ctx))) return rc;
  ctr.add_up();
  if (!nonmax) {  // PCL's branch: the whole response cloud, every record
    for (size_t i = 0; i < n; ++i) keypoints[i] = static_cast<int>(i);
    nkp = static_cast<uint32_t>(n);
  }
  *n_keypoints = nkp;
  inf.n_finite = static_cast<double>(nf);
  inf.n_candidates = static_cast<double>(ctr.sum[1]);
  inf.n_keypoints = static_cast<double>(nkp);
  inf.n_tied = static_cast<double>(ctr.sum[2]);
  inf.pair_tests = static_cast<double>(ctr.sum[0]);
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
  const FlannRadius fr(radius);
  const float r2 = fr.r2;
  int rc = radius_grid(ctx, xyz, n, stride, fr);
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
  PackedNormals nrm(normals, n, normal_stride);
  ScopedBuf<float> d_out;
  ScopedBuf<int> d_kp, d_msize;
  ScopedBuf<uint32_t> d_posof, d_mark, d_pos, d_list;
  ScopedBuf<uint16_t> d_rows;
  ScopedBuf<unsigned char> d_scratch;
  ScopedBuf<unsigned int> d_big;
  SlotCounters<2, kFpfhCtrSlots> ctr;
  const size_t sb = scan_scratch_bytes(nf + 1);
  HIPCK(nrm.reserve());
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
  HIPCK(ctr.reserve());
  HIPCK(nrm.upload(s));
  if (keypoints) HIPCK(hipMemcpyAsync(d_kp.p, keypoints, nk * sizeof(int), hipMemcpyHostToDevice, s));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  // records outside the union keep a zero row and size; records outside the grid have no position
  HIPCK(hipMemsetAsync(d_posof.p, 0xff, n * sizeof(uint32_t), s));
  HIPCK(hipMemsetAsync(d_rows.p, 0, nf * 33 * sizeof(uint16_t), s));
  HIPCK(hipMemsetAsync(d_msize.p, 0, nf * sizeof(int), s));
  HIPCK(hipMemsetAsync(d_big.p, 0, sizeof(unsigned int), s));
  HIPCK(ctr.zero(s));
  const GridView& g = ctx->aux.view;
  const int* kp = keypoints ? d_kp.p : nullptr;
  // 1. the union of the keypoints' sets, listed; 2. its SPFH rows; 3. the keypoints' histograms
  HIPCK(launch_fpfh_mark(g, nf, kp, nk, r2, d_posof.p, d_mark.p, d_pos.p, d_list.p, d_scratch.p, sb, d_big.p, ctr.dev.p, s));
  HIPCK(launch_fpfh_spfh(g, nf, d_list.p, d_pos.p + nf, nrm.dev.p, r2, d_rows.p, d_msize.p, d_big.p, ctr.dev.p, s));
  HIPCK(launch_fpfh_final(g, kp, nk, d_posof.p, r2, d_rows.p, d_msize.p, d_big.p, d_out.p, ctr.dev.p, s));
  if ((rc = sync(ctx))) return rc;
  const double t2 = now_ms();
  std::vector<float> ho(nk * 33);
  unsigned int too_big = 0;
  uint32_t n_rows = 0;
  HIPCK(hipMemcpyAsync(ho.data(), d_out.p, nk * 33 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCK(ctr.fetch(s));
  HIPCK(hipMemcpyAsync(&too_big, d_big.p, sizeof(too_big), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&n_rows, d_pos.p + nf, sizeof(n_rows), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  ctr.add_up();
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
  inf.pair_tests = static_cast<double>(ctr.sum[0]);
  inf.pair_features = static_cast<double>(ctr.sum[1]);
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

int mgicp_reject_ransac(mgicp_ctx* ctx, const float* src, size_t ns, size_t sstride, const float* tgt, size_t nt,
                        size_t tstride, const int* iq, const int* im, size_t m, double threshold, int max_iterations,
                        int refine, unsigned char* keep, size_t* n_keep, float best_T_cm[16], mgicp_ransac_info* info) {
  if (!ctx || !(threshold >= 0) || max_iterations < 0 || !n_keep || !best_T_cm || (m && !keep) ||
      bad_pairs(src, ns, sstride, tgt, nt, tstride, iq, im, m))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_ransac_info inf{};
  inf.final_error_threshold = threshold;
  // PCL's answer when it finds no model, the refine fails or fewer than 3 inliers remain: everything, identity
  auto keep_all = [&]() {
    if (m) std::memset(keep, 1, m);
    *n_keep = m;
    identity_cm(best_T_cm);
    inf.ms_total = now_ms() - t0;
    if (info) *info = inf;
    return MGICP_OK;
  };
  if (m < 3) return keep_all();
  hipStream_t s = ctx->stream;
  PairSet ps;
  MomentBufs mom;
  ScopedBuf<float> d_models, d_d2, d_d2p;
  ScopedBuf<unsigned int> d_counts;
  ScopedBuf<uint32_t> d_flag, d_pos, d_list[2];
  ScopedBuf<unsigned char> d_scratch;
  const size_t sb = scan_scratch_bytes(m + 1);
  int rc = ps.upload(ctx, src, ns, sstride, tgt, nt, tstride, iq, im, m);
  if (rc) return rc;
  HIPCK(mom.reserve(m));
  HIPCK(d_models.reserve(kRansacBatch * 12));
  HIPCK(d_counts.reserve(kRansacBatch));
  HIPCK(d_d2.reserve(m));
  HIPCK(d_d2p.reserve(m));
  HIPCK(d_flag.reserve(m + 1));
  HIPCK(d_pos.reserve(m + 1));
  HIPCK(d_list[0].reserve(m));
  HIPCK(d_list[1].reserve(m));
  HIPCK(d_scratch.reserve(sb));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  const double md = static_cast<double>(m);
  double pair_tests = 0.0;

  // sample_dist_thresh: the covariance of the correspondences' source points, each paired with itself
  double sums[15];
  const PairView self{ps.view.sxyz, ps.view.sxyz, ps.view.iq, ps.view.iq};
  if ((rc = mom.run(ctx, self, nullptr, m, sums))) return rc;
  const double sample_thresh = prealign::sample_dist_thresh(sums, md);

  // the selection of one model at one threshold: positions ascending, their (double)d2, into list buffer `buf`
  std::vector<float> h_d2;
  auto select = [&](const float T[12], double thr, int buf, std::vector<uint32_t>& list, std::vector<double>& d2) -> int {
    Xf34 X;
    std::copy(T, T + 12, X.m);
    HIPCK(launch_ransac_select(ps.view, m, X, prealign::strict_limit(thr * thr), d_flag.p, d_pos.p, d_d2.p, d_scratch.p,
                               sb, d_list[buf].p, d_d2p.p, s));
    uint32_t cnt = 0;
    HIPCK(hipMemcpyAsync(&cnt, d_pos.p + m, sizeof(cnt), hipMemcpyDeviceToHost, s));
    int r = sync(ctx);
    if (r) return r;
    pair_tests += md;
    list.resize(cnt);
    h_d2.resize(cnt);
    d2.resize(cnt);
    if (cnt) {
      HIPCK(hipMemcpyAsync(list.data(), d_list[buf].p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIPCK(hipMemcpyAsync(h_d2.data(), d_d2p.p, cnt * sizeof(float), hipMemcpyDeviceToHost, s));
      if ((r = sync(ctx))) return r;
    }
    for (uint32_t k = 0; k < cnt; ++k) d2[k] = static_cast<double>(h_d2[k]);
    return MGICP_OK;
  };

  // RandomSampleConsensus::computeModel: batches of hypotheses scored on the device, PCL's sequential loop
  // replayed over their counts.  A batch draws on past the loop's end; nothing after the loop draws
  prealign::Sampler sampler(m);
  const int batch = std::max(1, std::min(ctx->ransac_batch, kRansacBatch));
  const float lim = prealign::strict_limit(threshold * threshold);
  const double log_probability = std::log(1.0 - 0.99);
  const unsigned max_skip = static_cast<unsigned>(max_iterations) * 10u;
  const unsigned skipped = 0;  // three points always give a registration model
  int iterations = 0;
  long long best = -static_cast<long long>(INT32_MAX);
  double k = 1.0;
  bool have_model = false, ended = false;
  float best_model[12];
  std::vector<float> models(static_cast<size_t>(kRansacBatch) * 12);
  unsigned int counts[kRansacBatch];
  while (!ended && iterations < k && skipped < max_skip) {
    int nb = 0;
    bool ran_dry = false;
    for (; nb < batch; ++nb) {
      int smp[3];
      if (!sampler.sample(ps.hs.data(), iq, sample_thresh, smp)) {
        ran_dry = true;
        break;
      }
      float sp[3][3], tp[3][3];
      for (int j = 0; j < 3; ++j) {
        std::memcpy(sp[j], &ps.hs[3 * static_cast<size_t>(iq[smp[j]])], 12);
        std::memcpy(tp[j], &ps.ht[3 * static_cast<size_t>(im[smp[j]])], 12);
      }
      double s3[15];
      prealign::sums_of_three(sp, tp, s3);
      prealign::model_from_sums(s3, 3.0, &models[12 * static_cast<size_t>(nb)]);
    }
    if (nb) {
      HIPCK(hipMemcpyAsync(d_models.p, models.data(), static_cast<size_t>(nb) * 12 * sizeof(float), hipMemcpyHostToDevice, s));
      HIPCK(launch_ransac_score(ps.view, m, d_models.p, nb, lim, d_counts.p, s));
      HIPCK(hipMemcpyAsync(counts, d_counts.p, sizeof(counts), hipMemcpyDeviceToHost, s));
      if ((rc = sync(ctx))) return rc;
      inf.n_hypotheses += nb;
      pair_tests += md * nb;
    }
    for (int j = 0; j < nb; ++j) {
      if (!(iterations < k && skipped < max_skip)) {
        ended = true;
        break;
      }
      const long long c = counts[j];
      if (c > best) {
        best = c;
        have_model = true;
        std::copy(&models[12 * static_cast<size_t>(j)], &models[12 * static_cast<size_t>(j)] + 12, best_model);
        const double w = static_cast<double>(best) * (1.0 / md);
        double p_no_outliers = 1.0 - std::pow(w, 3.0);
        p_no_outliers = std::max(std::numeric_limits<double>::epsilon(), p_no_outliers);
        p_no_outliers = std::min(1.0 - std::numeric_limits<double>::epsilon(), p_no_outliers);
        k = log_probability / std::log(p_no_outliers);
      }
      ++iterations;
      if (iterations > max_iterations) {
        ended = true;
        break;
      }
    }
    if (ran_dry) ended = true;  // the loop's next getSamples comes back empty
  }
  inf.n_iterations = iterations;
  inf.n_skipped = skipped;
  auto finish_times = [&]() {
    inf.pair_tests = pair_tests;
    inf.ms_device = now_ms() - t1;
  };
  if (!have_model) {
    finish_times();
    return keep_all();
  }
  std::vector<uint32_t> inliers, prev, fresh;
  std::vector<double> d2;
  if ((rc = select(best_model, threshold, 0, inliers, d2))) return rc;
  inf.n_inliers_ransac = static_cast<double>(inliers.size());
  float model[12];
  std::copy(best_model, best_model + 12, model);
  bool ok = true;
  if (refine) {
    // SampleConsensus::refineModel(3.0, 1000), statement for statement; `fresh` is PCL's new_inliers
    const double thr2 = threshold * threshold;
    double error_threshold = threshold;
    unsigned rounds = 0;
    bool changed = false, oscillating = false;
    std::vector<size_t> sizes;
    float cur[12];
    std::copy(best_model, best_model + 12, cur);
    prev = inliers;
    int pb = 0;  // the device list buffer that holds prev
    do {
      inf.n_refine_rounds += 1;
      if (!prev.empty()) {
        if ((rc = mom.run(ctx, ps.view, d_list[pb].p, prev.size(), sums))) return rc;
        prealign::model_from_sums(sums, static_cast<double>(prev.size()), cur);
      }
      sizes.push_back(prev.size());
      if ((rc = select(cur, error_threshold, 1 - pb, fresh, d2))) return rc;
      if (fresh.empty()) {
        ++rounds;
        if (rounds >= 1000) break;
        continue;
      }
      const size_t mid = d2.size() >> 1;
      std::nth_element(d2.begin(), d2.begin() + static_cast<std::ptrdiff_t>(mid), d2.end());
      const double variance = 2.1981 * d2[mid];
      error_threshold = std::sqrt(std::min(thr2, 9.0 * variance));
      changed = false;
      std::swap(prev, fresh);
      pb = 1 - pb;
      if (fresh.size() != prev.size()) {
        const size_t z = sizes.size();
        if (z >= 4 && sizes[z - 1] == sizes[z - 3] && sizes[z - 2] == sizes[z - 4]) {
          oscillating = true;
          break;
        }
        changed = true;
        continue;
      }
      changed = prev != fresh;
    } while (changed && ++rounds < 1000);
    inf.final_error_threshold = error_threshold;
    if (fresh.empty()) ok = false;
    else if (oscillating) ok = true;  // inliers and model stay the loop's
    else if (!changed) {
      inliers.swap(fresh);
      std::copy(cur, cur + 12, model);
    } else ok = false;
  }
  finish_times();
  inf.n_inliers_final = ok ? static_cast<double>(inliers.size()) : 0.0;
  if (!ok || inliers.size() < 3) return keep_all();
  std::memset(keep, 0, m);
  for (uint32_t p : inliers) keep[p] = 1;
  *n_keep = inliers.size();
  rows_to_cm(model, best_T_cm);
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_reject_one_to_one(mgicp_ctx* ctx, const int* im, const float* distance, size_t m, size_t nt, int* order,
                            size_t* n_keep, double* ms_device) {
  if (!ctx || !n_keep || (m && (!im || !distance || !order)) || m > size_t(INT32_MAX) || nt > size_t(INT32_MAX))
    return MGICP_E_INVALID;
  std::vector<float> hd(m);
  for (size_t i = 0; i < m; ++i) {
    if ((im[i] >= 0 && static_cast<size_t>(im[i]) >= nt) || !(distance[i] >= 0.f)) return MGICP_E_INVALID;
    hd[i] = distance[i] == 0.f ? 0.f : distance[i];  // -0.0 orders as 0
  }
  HIPCK(hipSetDevice(ctx->device));
  *n_keep = 0;
  if (ms_device) *ms_device = 0.0;
  if (m == 0) return MGICP_OK;
  hipStream_t s = ctx->stream;
  ScopedBuf<int> d_im, d_order;
  ScopedBuf<float> d_dist;
  ScopedBuf<unsigned long long> d_best;
  ScopedBuf<uint32_t> d_flag, d_pos;
  ScopedBuf<unsigned char> d_scratch;
  const size_t sb = scan_scratch_bytes(nt + 1);
  HIPCK(d_im.reserve(m));
  HIPCK(d_order.reserve(m));
  HIPCK(d_dist.reserve(m));
  HIPCK(d_best.reserve(std::max<size_t>(nt, 1)));
  HIPCK(d_flag.reserve(nt + 1));
  HIPCK(d_pos.reserve(nt + 1));
  HIPCK(d_scratch.reserve(sb));
  HIPCK(hipMemcpyAsync(d_im.p, im, m * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(d_dist.p, hd.data(), m * sizeof(float), hipMemcpyHostToDevice, s));
  int rc = sync(ctx);
  if (rc) return rc;
  const double t1 = now_ms();
  HIPCK(launch_one_to_one(d_im.p, d_dist.p, m, nt, d_best.p, d_flag.p, d_pos.p, d_scratch.p, sb, d_order.p, s));
  if ((rc = sync(ctx))) return rc;
  if (ms_device) *ms_device = now_ms() - t1;
  uint32_t cnt = 0;
  HIPCK(hipMemcpyAsync(order, d_order.p, m * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&cnt, d_pos.p + nt, sizeof(cnt), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  *n_keep = cnt;
  return MGICP_OK;
}

int mgicp_estimate_rigid_svd(mgicp_ctx* ctx, const float* src, size_t ns, size_t sstride, const float* tgt, size_t nt,
                             size_t tstride, const int* iq, const int* im, size_t m, float T_cm[16],
                             mgicp_svd_info* info) {
  if (!ctx || !T_cm || bad_pairs(src, ns, sstride, tgt, nt, tstride, iq, im, m)) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_svd_info inf{};
  identity_cm(T_cm);
  if (info) *info = inf;
  if (m == 0) return MGICP_OK;
  PairSet ps;
  MomentBufs mom;
  int rc = ps.upload(ctx, src, ns, sstride, tgt, nt, tstride, iq, im, m);
  if (rc) return rc;
  HIPCK(mom.reserve(m));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  if ((rc = mom.run(ctx, ps.view, nullptr, m, inf.sums))) return rc;
  inf.ms_device = now_ms() - t1;
  float T[12];
  prealign::model_from_sums(inf.sums, static_cast<double>(m), T);
  rows_to_cm(T, T_cm);
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_normal_clusters(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, const float* normals,
                          size_t normal_stride, double tolerance, double eps_angle, size_t min_size, size_t max_size,
                          int* labels, int* indices, size_t* offsets, mgicp_normal_cluster_info* info) {
  if (!ctx || !(tolerance >= 0) || !(eps_angle >= 0) || !offsets || (n && (!xyz || !normals || !labels || !indices)) ||
      stride < 12 || (stride % 4) || normal_stride < 12 || (normal_stride % 4) || n > size_t(INT32_MAX))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  mgicp_normal_cluster_info inf{};
  if (info) *info = inf;
  offsets[0] = 0;
  if (n == 0) return MGICP_OK;
  const FlannRadius fr(tolerance);
  const float r2 = fr.r2;
  // the forced tolerance / 2 grid of the Euclidean clustering (the walks are exact for any edge)
  int rc = aux_grid(ctx, xyz, n, stride, r2 > 0.f ? std::min(0.5 * fr.reach, 1e30) : 0.0);
  if (rc) return rc;
  std::fill(labels, labels + n, -1);
  std::fill(offsets, offsets + n + 1, size_t(0));
  const size_t nf = ctx->aux.n;
  if (nf == 0) return MGICP_OK;
  const float c_min = normal_cluster_c_min(eps_angle);
  const GridView& g = ctx->aux.view;
  hipStream_t s = ctx->stream;
  int bits = 1;
  while ((size_t(1) << bits) < n && bits < 32) ++bits;
  const size_t sb = sort_scratch_bytes(nf, bits);
  PackedNormals nrm(normals, n, normal_stride);
  ScopedBuf<float4> d_nrm;
  ScopedBuf<uint32_t> d_owner, d_order, d_front[2];
  ScopedBuf<unsigned int> d_count;
  ScopedBuf<NcState> d_state;
  SlotCounters<1, kNcCtrSlots> ctr;
  HIPCK(nrm.reserve());
  HIPCK(d_nrm.reserve(nf));
  HIPCK(d_owner.reserve(nf));
  HIPCK(d_order.reserve(nf));
  HIPCK(d_front[0].reserve(nf));
  HIPCK(d_front[1].reserve(nf));
  HIPCK(d_count.reserve(2));
  HIPCK(d_state.reserve(1));
  HIPCK(ctr.reserve());
  HIPCK(ctx->cc_members.reserve(nf));
  HIPCK(ctx->keys.reserve(nf));
  HIPCK(ctx->keys_sorted.reserve(nf));
  HIPCK(ctx->vals.reserve(nf));
  HIPCK(ctx->scratch.reserve(sb));
  HIPCK(nrm.upload(s));
  if ((rc = sync(ctx))) return rc;
  const double t1 = now_ms();
  HIPCK(hipMemsetAsync(d_state.p, 0, sizeof(NcState), s));
  HIPCK(hipMemsetAsync(d_count.p, 0, 2 * sizeof(unsigned int), s));
  HIPCK(ctr.zero(s));
  HIPCK(launch_nc_begin(g, ctx->aux.perm.p, nf, nrm.dev.p, d_nrm.p, d_owner.p, d_order.p, s));
  // small path until a round hands over, that round's levels on the wide path, and again: at most nf
  // rounds and nf levels in all, as every one of them claims a record
  const uint32_t limit = static_cast<uint32_t>(ctx->nc_small_limit);
  NcState st{};
  size_t levels = 0, wide_rounds = 0;
  for (size_t turn = 0; turn <= nf; ++turn) {
    HIPCK(launch_nc_small(g, nf, d_nrm.p, d_order.p, d_owner.p, r2, c_min, limit, d_front[0].p, d_state.p, s));
    HIPCK(hipMemcpyAsync(&st, d_state.p, sizeof(st), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    if (st.status == 0) break;
    ++wide_rounds;
    const float* sn = &nrm.host[3 * static_cast<size_t>(st.seed)];
    // a level: one launch and the read-back of its count through the pinned scratch.  Both counters are zero
    // here: a round ends on a zero count, and its last launch zeroed the other one
    unsigned int cnt = st.count;
    int cur = 0;
    while (cnt && levels <= nf) {
      if (cnt > nf) return fail(ctx, MGICP_E_HIP, "normal clusters: a frontier larger than the cloud");
      HIPCK(launch_nc_expand(g, d_nrm.p, d_owner.p, d_front[cur].p, cnt, r2, sn, c_min, st.seed, d_front[1 - cur].p,
                             d_count.p, cur, ctr.dev.p, s));
      HIPCK(hipMemcpyAsync(ctx->h_small, d_count.p + cur, sizeof(cnt), hipMemcpyDeviceToHost, s));
      if ((rc = sync(ctx))) return rc;
      std::memcpy(&cnt, ctx->h_small, sizeof(cnt));
      ++levels;
      cur = 1 - cur;
    }
  }
  if (st.status != 0) return fail(ctx, MGICP_E_HIP, "normal clusters: the rounds did not end");
  HIPCK(launch_nc_emit(g, ctx->aux.perm.p, nf, d_owner.p, ctx->keys.p, ctx->vals.p, s));
  HIPCK(launch_sort_pairs(ctx->scratch.p, sb, ctx->keys.p, ctx->keys_sorted.p, ctx->vals.p, ctx->cc_members.p, nf, bits, s));
  if ((rc = sync(ctx))) return rc;
  const double t2 = now_ms();
  std::vector<uint32_t> hk(nf), hv(nf);
  HIPCK(hipMemcpyAsync(hk.data(), ctx->keys_sorted.p, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(hv.data(), ctx->cc_members.p, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCK(ctr.fetch(s));
  if ((rc = sync(ctx))) return rc;
  ctr.add_up();
  // runs of equal seeds come in ascending seed, PCL's output order (the free function does not sort by size)
  const size_t lo = std::max<size_t>(min_size, 1), hi = max_size ? max_size : SIZE_MAX;
  size_t off = 0, nc = 0, rounds = 0;
  for (size_t i = 0; i < nf;) {
    size_t j = i + 1;
    while (j < nf && hk[j] == hk[i]) ++j;
    ++rounds;
    if (j - i >= lo && j - i <= hi) {
      offsets[nc] = off;
      for (size_t m = i; m < j; ++m) {
        indices[off++] = static_cast<int>(hv[m]);
        labels[hv[m]] = static_cast<int>(nc);
      }
      ++nc;
    }
    i = j;
  }
  for (size_t c = nc; c <= n; ++c) offsets[c] = off;
  if (rounds != st.rounds) return fail(ctx, MGICP_E_HIP, "normal clusters: the rounds run and the sets found disagree");
  inf.n_rounds = static_cast<double>(rounds);
  inf.n_clusters = static_cast<double>(nc);
  inf.n_clustered_points = static_cast<double>(off);
  inf.n_levels = static_cast<double>(levels);
  inf.n_wide_rounds = static_cast<double>(wide_rounds);
  inf.pair_tests = static_cast<double>(ctr.sum[0] + st.walked);
  inf.ms_grid = t1 - t0;
  inf.ms_device = t2 - t1;
  inf.ms_total = now_ms() - t0;
  if (info) *info = inf;
  return MGICP_OK;
}

int mgicp_dominant_normals(mgicp_ctx* ctx, const float* normals, size_t n, size_t normal_stride, const int* indices,
                           const size_t* offsets, size_t n_clusters, float* out, double* ms_device) {
  if (!ctx || (n && !normals) || normal_stride < 12 || (normal_stride % 4) || n > size_t(INT32_MAX) ||
      n_clusters > size_t(INT32_MAX) || (n_clusters && (!indices || !offsets || !out)))
    return MGICP_E_INVALID;
  if (ms_device) *ms_device = 0.0;
  if (n_clusters == 0) return MGICP_OK;
  // every cluster non-empty, every member a record; the blocks of 256 entries (size + 1 of them per cluster)
  std::vector<uint32_t> blk_first(n_clusters + 1), blk_cluster;
  std::vector<unsigned long long> off64(n_clusters + 1);
  for (size_t c = 0; c < n_clusters; ++c) {
    if (offsets[c + 1] <= offsets[c]) return fail(ctx, MGICP_E_INVALID, "dominant normals: an empty cluster");
    const size_t nb = (offsets[c + 1] - offsets[c] + 1 + 255) / 256;
    if (blk_cluster.size() + nb > size_t(INT32_MAX)) return MGICP_E_INVALID;
    blk_first[c] = static_cast<uint32_t>(blk_cluster.size());
    blk_cluster.insert(blk_cluster.end(), nb, static_cast<uint32_t>(c));
    off64[c] = offsets[c] - offsets[0];
  }
  blk_first[n_clusters] = static_cast<uint32_t>(blk_cluster.size());
  const size_t total = offsets[n_clusters] - offsets[0];
  off64[n_clusters] = total;
  const int* idx = indices + offsets[0];
  for (size_t i = 0; i < total; ++i)
    if (idx[i] < 0 || static_cast<size_t>(idx[i]) >= n)
      return fail(ctx, MGICP_E_INVALID, "dominant normals: member index outside [0, n)");
  HIPCK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  PackedNormals nrm(normals, n, normal_stride);
  ScopedBuf<int> d_idx;
  ScopedBuf<unsigned long long> d_off;
  ScopedBuf<uint32_t> d_bc, d_bf;
  ScopedBuf<double> d_partial;
  ScopedBuf<float> d_out;
  std::vector<float> ho(3 * n_clusters);
  HIPCK(nrm.reserve());
  HIPCK(d_idx.reserve(total));
  HIPCK(d_off.reserve(n_clusters + 1));
  HIPCK(d_bc.reserve(blk_cluster.size()));
  HIPCK(d_bf.reserve(n_clusters + 1));
  HIPCK(d_partial.reserve(blk_cluster.size() * kRedVals));
  HIPCK(d_out.reserve(3 * n_clusters));
  // the copies read this call's vectors: the stream is synchronised before any of them goes away
  hipError_t e = nrm.upload(s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_idx.p, idx, total * sizeof(int), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, off64.data(), off64.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_bc.p, blk_cluster.data(), blk_cluster.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_bf.p, blk_first.data(), blk_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
  int rc = sync(ctx);
  HIPCK(e);
  if (rc) return rc;
  const double t1 = now_ms();
  e = launch_dominant_normals(nrm.dev.p, d_idx.p, d_off.p, d_bc.p, d_bf.p, blk_cluster.size(), n_clusters, d_partial.p,
                              d_out.p, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ho.data(), d_out.p, ho.size() * sizeof(float), hipMemcpyDeviceToHost, s);
  rc = sync(ctx);
  HIPCK(e);
  if (rc) return rc;
  if (ms_device) *ms_device = now_ms() - t1;
  std::copy(ho.begin(), ho.end(), out);
  return MGICP_OK;
}

int mgicp_debug_score_models(mgicp_ctx* ctx, const float* src, size_t ns, size_t sstride, const float* tgt, size_t nt,
                             size_t tstride, const int* iq, const int* im, size_t m, const float* models_cm,
                             int n_models, double threshold, int* counts) {
  if (!ctx || !(threshold >= 0) || n_models < 0 || (n_models && (!models_cm || !counts)) ||
      bad_pairs(src, ns, sstride, tgt, nt, tstride, iq, im, m))
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  PairSet ps;
  ScopedBuf<float> d_models;
  ScopedBuf<unsigned int> d_counts;
  int rc = ps.upload(ctx, src, ns, sstride, tgt, nt, tstride, iq, im, m);
  if (rc) return rc;
  HIPCK(d_models.reserve(kRansacBatch * 12));
  HIPCK(d_counts.reserve(kRansacBatch));
  const int batch = std::max(1, std::min(ctx->ransac_batch, kRansacBatch));
  const float lim = prealign::strict_limit(threshold * threshold);
  std::vector<float> rows(static_cast<size_t>(kRansacBatch) * 12);
  unsigned int got[kRansacBatch];
  for (int b0 = 0; b0 < n_models; b0 += batch) {
    const int nb = std::min(batch, n_models - b0);
    for (int b = 0; b < nb; ++b) {
      const Xf34 x = Mat4::from_cm(models_cm + 16 * static_cast<size_t>(b0 + b)).xf();
      std::copy(x.m, x.m + 12, &rows[12 * static_cast<size_t>(b)]);
    }
    HIPCK(hipMemcpyAsync(d_models.p, rows.data(), static_cast<size_t>(nb) * 12 * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCK(launch_ransac_score(ps.view, m, d_models.p, nb, lim, d_counts.p, s));
    HIPCK(hipMemcpyAsync(got, d_counts.p, sizeof(got), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    for (int b = 0; b < nb; ++b) counts[b0 + b] = static_cast<int>(got[b]);
  }
  return sync(ctx);
}

}  // extern "C"
