// mgicp_fod.hip -- the filter and detector calls beside the alignment (include/mi355x_gicp.h): point
// transforms, cloud resolution, the radius filter, segment differences, Euclidean clustering and the
// voxel grid.  The feature calls of the initial alignment are in mgicp_features.hip.
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
  // FLANN's radius over the tolerance.  0 links nothing (not even duplicates): singletons
  const FlannRadius fr(tolerance);
  const float r2 = fr.r2;
  const bool link = r2 > 0.f;
  // non-finite records join no cluster: grid (and forest) over the finite points, label -1 for the rest
  int rc = aux_grid(ctx, xyz, n, stride, link ? 0.5 * fr.reach : 0.0);
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
