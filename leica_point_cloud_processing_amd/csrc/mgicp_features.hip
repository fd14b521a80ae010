// mgicp_features.hip -- the feature calls of the initial alignment (include/mi355x_gicp.h): radius normals,
// boundary points, Harris keypoints, FPFH descriptors and feature correspondences.  Host code only: the
// kernels and their launchers are in mgicp_kernels.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mgicp_ctx.hpp"

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

}  // extern "C"
