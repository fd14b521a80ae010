// mgicp_clouds.hip -- a cloud on the device: its upload, its row-sorted uniform grid (build_grid), the
// Morton query order, the k-NN covariances and their scheduling (the head start on the aux stream, the
// joins, the lazy source mode), and the process-wide target cache.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "host_upload.hpp"
#include "mgicp_ctx.hpp"

using namespace mgicp;

bool (*mgicp::g_oom_evict)() = nullptr;
TargetCache mgicp::g_tcache[64];  // r05 target cache: one entry per device

namespace {

constexpr double kDefaultOccupancy = 10.0;          // mean points per non-empty cell (A/B: profiles/r01/ab_tocc)
constexpr size_t kSketchOffset = size_t(32) << 10;  // the grid sizing sketch's registers in h_small (16 KiB)
constexpr size_t kMaxCells = size_t(1) << 29;       // dense cell table cap (2 GiB of uint32)
// rings the lazy source's head-start k-NN searches before leaving a point to the lazy pass (caps 2-4
// measured equal with the wave-per-point lazy pass, profiles/r06)
constexpr int kAsyncRingCap = 4;
constexpr unsigned int kWaveKnnMax = 65536;  // r06: lazy / hand-off lists up to this size run knn_wave_kernel

// MGICP_KNN_STATS=1: k-NN hand-off counts per covariance pass on stderr (diagnostic)
// (read at every covariance pass: tests switch it per context)
bool knn_stats_on() { return std::getenv("MGICP_KNN_STATS") != nullptr; }

template <class T>
void swap_buf(DevBuf<T>& a, DevBuf<T>& b) {  // the device memory changes hands; each side keeps its graveyard
  std::swap(a.p, b.p);
  std::swap(a.cap, b.cap);
}

// the target's device state: every buffer a grid, its covariances and its cell lists live in
template <class F>
void each_target_buf(Cloud& a, Cloud& b, F&& f) {
  f(a.orig, b.orig); f(a.pts, b.pts); f(a.perm, b.perm); f(a.cell_start, b.cell_start);
  f(a.empty_dist, b.empty_dist); f(a.seed, b.seed); f(a.seed_scratch, b.seed_scratch);
  f(a.pairs, b.pairs); f(a.cov, b.cov);
}
void tcache_clear_locked(TargetCache& c) {
  Cloud none;
  each_target_buf(c.t, none, [](auto& x, auto&) { x.release(); });
  c.vl_cell.release();
  c.vl_pool.release();
  c.vl_ctr.release();
  c.valid = false;
}
bool tcache_evict_current() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  TargetCache& c = g_tcache[dev & 63];
  std::unique_lock<std::mutex> lk(c.mu, std::try_to_lock);  // never from inside the cache's own lock
  if (!lk.owns_lock() || (!c.valid && !c.t.orig.p && !c.vl_pool.p)) return false;
  tcache_clear_locked(c);
  return true;
}
struct OomHookInit {
  OomHookInit() { g_oom_evict = &tcache_evict_current; }
} g_oom_hook_init;

// The target's grid and covariance arrays change sides (context <-> cache): the device buffers and the
// fields that describe them.  What the receiving side decides itself (n, dirty, have_cov and its range,
// fresh_grid, the want_* / drop_nonfinite flags) is set by the caller.
void swap_target_state(Cloud& a, Cloud& b) {
  each_target_buf(a, b, [](auto& x, auto& y) { swap_buf(x, y); });
  std::swap(a.cov_stride, b.cov_stride);
  std::swap(a.n_built, b.n_built);
  std::swap(a.lo, b.lo);
  std::swap(a.hi, b.hi);
  std::swap(a.view, b.view);  // the same device memory, now the other side's
  std::swap(a.ncells, b.ncells);
}
// the same for the 1-NN cell lists of a target (A, B: the context or the cache entry)
template <class A, class B>
void swap_list_state(A& a, B& b) {
  swap_buf(a.vl_cell, b.vl_cell);
  swap_buf(a.vl_pool, b.vl_pool);
  swap_buf(a.vl_ctr, b.vl_ctr);
  std::swap(a.vl, b.vl);
  std::swap(a.vl_alloc, b.vl_alloc);
  std::swap(a.vl_off, b.vl_off);
  std::swap(a.vl_ncells, b.vl_ncells);
  std::swap(a.vl_epoch, b.vl_epoch);
  std::swap(a.vl_groups, b.vl_groups);
}

// The 1-NN sweeps' extras of a built grid (target): empty-space + seed map, the
// pair-interleaved copy -- queued on the main stream, no host wait.  r06: set_target's head start queues
// the target's k-NN (which needs none of them) BEFORE these, so the 0.7-0.8 ms of the empty map at C4 run
// beside the k-NN instead of in front of it (the target's k-NN is the cold first align's long pole).
int build_grid_extras(mgicp_ctx* ctx, Cloud& cl) {
  GridView& g = cl.view;
  hipStream_t s = ctx->stream;
  const size_t nc = cl.ncells, n = cl.n;
  if (cl.want_empty_map) {
    HIPCK(cl.empty_dist.reserve(nc));
    HIPCK(ctx->scratch.reserve(nc));
    if (cl.want_seed_map) {
      HIPCK(cl.seed.reserve(nc));
      HIPCK(cl.seed_scratch.reserve(nc));
    }
    HIPCK(launch_empty_map(cl.cell_start.p, g.nx, g.ny, g.nz, cl.empty_dist.p, ctx->scratch.p, s,
                           cl.want_seed_map ? cl.seed.p : nullptr, cl.want_seed_map ? cl.seed_scratch.p : nullptr,
                           &g));
    MGICP_TRACE_AT("grid: empty map queued");
    g.empty_dist = cl.empty_dist.p;
    if (cl.want_seed_map) g.seed = cl.seed.p;
  }
  if (&cl == &ctx->tgt) {  // the wave-uniform 1-NN scan reads the target's pair copy
    HIPCK(cl.pairs.reserve(2 * pair_count(n)));
    HIPCK(launch_pairs(cl.pts.p, n, cl.pairs.p, s));
    g.pairs = cl.pairs.p;
  }
  return MGICP_OK;
}

// Morton order of points [p0, p0 + n) of a grid-sorted cloud: a stable sort of 30-bit Morton codes
// over the cloud's bbox.  Query order of the k-NN / 1-NN kernels (a wave's queries then form a
// compact 3-D patch); results stay indexed by grid-sorted position.  false on failure.
bool morton_perm(mgicp_ctx* ctx, const Cloud& c, size_t p0, size_t n, DevBuf<uint32_t>& out, bool aux) {
  hipStream_t s = aux ? ctx->aux_stream : ctx->stream;
  DevBuf<uint32_t>& keys = aux ? ctx->aq_keys : ctx->keys;
  DevBuf<uint32_t>& keys_sorted = aux ? ctx->aq_keys_sorted : ctx->keys_sorted;
  DevBuf<uint32_t>& vals = aux ? ctx->aq_vals : ctx->vals;
  DevBuf<unsigned char>& scratch = aux ? ctx->aq_scratch : ctx->scratch;
  float ext = 0.f;
  for (int d = 0; d < 3; ++d) ext = std::max(ext, c.hi[d] - c.lo[d]);
  const float inv = ext > 0.f ? 1024.0f / (ext * 1.0001f) : 0.f;
  if (out.reserve(n) != hipSuccess || keys.reserve(n) != hipSuccess ||
      keys_sorted.reserve(n) != hipSuccess || vals.reserve(n) != hipSuccess)
    return false;
  const size_t sb = sort_scratch_bytes(n, 30);
  if (scratch.reserve(sb) != hipSuccess) return false;
  return launch_morton_keys(c.pts.p, p0, n, c.lo, inv, keys.p, vals.p, s) == hipSuccess &&
         launch_sort_pairs(scratch.p, sb, keys.p, keys_sorted.p, vals.p, out.p, n, 30, s) == hipSuccess;
}

// the covariances started by cov_prep_async: wait for the aux stream, then hand the points the
// logged kernel left (log overflow, ties at the k-th distance) to the register-list kernel on the
// main stream -- the same two launches as compute_cov
int cov_join(mgicp_ctx* ctx, bool tgt) {
  bool& pending = tgt ? ctx->tgt_cov_pending : ctx->src_cov_pending;
  if (!pending) return MGICP_OK;
  pending = false;
  Cloud& c = tgt ? ctx->tgt : ctx->src;
  // this cloud's launches only (the logged k-NN pass and its hand-off, chained on the aux stream):
  // the main stream waits for them on the device, the host does not
  HIPCK(hipStreamWaitEvent(ctx->stream, ctx->aux_ev[tgt ? 0 : 1], 0));
  if (ctx->knn_logged && knn_stats_on()) {  // as compute_cov reports it
    unsigned int nfb = 0;
    HIPCK(hipMemcpyAsync(ctx->h_small, ctx->aux_cnt.p + (tgt ? 0 : 1), sizeof(nfb), hipMemcpyDeviceToHost, ctx->stream));
    HIPCK(hipStreamSynchronize(ctx->stream));
    std::memcpy(&nfb, ctx->h_small, sizeof(nfb));
    ctx->knn_fallbacks = nfb;
    std::fprintf(stderr, "[knn] %zu points, %u left to the register-list kernel\n", c.n, nfb);
  }
  if (!tgt && ctx->src_async_lazy) return MGICP_OK;  // the points it gave up on: computed if a sweep accepts them
  c.have_cov = true;
  c.cov_p0 = 0;
  c.cov_p1 = c.n;
  return MGICP_OK;
}

// set_target's / set_source's head start (single rank, eager target covariances, not profiling): the
// cloud's grid now (its host round trips), then its k-NN covariances on the aux stream -- the
// target's overlap the source's upload and grid build, the source's the first 1-NN sweep.  Any
// failure leaves the cloud for prepare, which reports it as before.
int cov_prep_async(mgicp_ctx* ctx, bool tgt) {
  Cloud& c = tgt ? ctx->tgt : ctx->src;
  if (!ctx->async_tgt || !ctx->aux_stream || ctx->nranks != 1 || ctx->comm || ctx->have_shm || ctx->profiling ||
      static_cast<size_t>(ctx->prm.k) > c.n)
    return MGICP_OK;
  // r06: the grid's core (sorted points, cell starts) only; the 1-NN extras are queued after the k-NN
  if (build_grid(ctx, c, true) != MGICP_OK) return MGICP_OK;
  if (c.n < static_cast<size_t>(ctx->prm.k)) return build_grid_extras(ctx, c);
  HIPCK(c.cov.reserve(3 * c.n));
  c.cov_stride = c.n;
  // the source in the lazy mode: a ring-capped launch (a point whose 20 neighbours lie beyond the
  // cap -- scan clutter, debris -- is left to the lazy pass, which computes it only if a sweep accepts
  // it; r04 C4F: the uncapped head start spent ~40 ms on them); its points are marked in cov_ok
  const bool capped = !tgt && ctx->lazy_src_cov && ctx->knn_logged;
  // r06 fix: the flag belongs to the SOURCE's launch -- the target's head start (set_target after
  // set_source on a context whose old target let the source start first) must not clear it, or the
  // source's join would mark the points its capped launch gave up on as computed (stale covariances)
  if (!tgt) ctx->src_async_lazy = capped;
  if (capped) {
    HIPCK(ctx->cov_ok.reserve(c.n));
    HIPCK(ctx->cov_need.reserve(c.n));
    HIPCK(hipMemsetAsync(ctx->cov_ok.p, 0, c.n, ctx->stream));
    ctx->src_lazy_ready = true;
    ctx->src_lazy_p0 = 0;
    ctx->src_lazy_p1 = c.n;
  }
  if (ctx->knn_logged) {
    HIPCK((tgt ? ctx->knn_fb : ctx->knn_fb2).reserve(c.n));
    HIPCK(ctx->aux_cnt.reserve(2));
    HIPCK(hipMemsetAsync(ctx->aux_cnt.p + (tgt ? 0 : 1), 0, sizeof(unsigned int), ctx->stream));
  }
  // the grid (and the count) before the aux stream reads them: a device-side dependency (r06; r04-r05
  // waited on the host)
  HIPCK(hipEventRecord(ctx->aux_ev[3], ctx->stream));
  HIPCK(hipStreamWaitEvent(ctx->aux_stream, ctx->aux_ev[3], 0));
  // the source's Morton query order is sorted on the aux stream ahead of its k-NN, so the main stream stays
  // empty for set_target's upload (r05: queued behind a main-stream sort that shares the CUs with the k-NN,
  // the target's copies waited ~2 ms)
  if (!tgt && !ctx->qperm_valid && !ctx->qperm_aux) {
    const size_t p0 = ctx->shard_p0(), ns = ctx->shard_p1() - p0;
    if (ns > 0 && morton_perm(ctx, c, p0, ns, ctx->qperm, true)) {
      HIPCK(hipEventRecord(ctx->aux_ev[2], ctx->aux_stream));
      ctx->qperm_valid = true;
      ctx->qperm_aux = true;
    }
  }
  HIPCK(launch_knn_cov(c.view, ctx->prm.k, ctx->prm.gicp_eps, 0, c.n, c.cov3(), nullptr,
                       ctx->knn_logged ? (tgt ? ctx->knn_fb.p : ctx->knn_fb2.p) : nullptr,
                       ctx->knn_logged ? ctx->aux_cnt.p + (tgt ? 0 : 1) : nullptr, ctx->aux_stream,
                       capped ? kAsyncRingCap : -1, capped ? ctx->cov_ok.p : nullptr,
                       ctx->knn_logged ? 2 * std::max(ctx->cus, 1) : 0, ctx->knn_wave));
  HIPCK(hipEventRecord(ctx->aux_ev[tgt ? 0 : 1], ctx->aux_stream));
  MGICP_TRACE_AT(tgt ? "head start: target k-NN queued" : "head start: source k-NN queued");
  (tgt ? ctx->tgt_cov_pending : ctx->src_cov_pending) = true;
  if (int rc = build_grid_extras(ctx, c)) return rc;  // the target's empty / seed map, pairs
  // r05: the source's 1-NN query order (a Morton sort of the shard) now, on the main stream beside the
  // covariances -- not inside the first align's loop
  if (!tgt && !ctx->qperm_aux) (void)query_perm(ctx);
  return MGICP_OK;
}

}  // namespace

int mgicp::cov_join_all(mgicp_ctx* ctx) {
  const int rc = cov_join(ctx, true);
  return rc ? rc : cov_join(ctx, false);
}

// after a set_*: the head start of the cloud just set -- its grid now (its host round trips), then its
// k-NN covariances on the aux stream.  r06: the source's grid is sized from the source alone (like the
// target's from the target), so its head start runs at set_source, whatever the order of the set_* calls
// and whether a target exists yet: the reference sets the source first (GICPAlignment.cpp:89-90), and
// the source's k-NN now overlaps set_target's upload and grid build.  (r04-r05 started the source's grid
// from the target's cell size, so a source set first waited for set_target; that dependency rested on a
// C4F trajectory flip later traced to a bug -- set_target's head start cleared the source's ring-cap flag
// -- not to the summation order, which the r06 ledger shows does not move C2F / C4F / C5:
// DESIGN.md "Summation-order ledger".)  The target's covariances are joined only before the first
// compaction, so they run beside the first 1-NN sweep.
int mgicp::cov_prep_async_all(mgicp_ctx* ctx) {
  int rc = MGICP_OK;
  if (ctx->tgt.dirty && (rc = cov_prep_async(ctx, true))) return rc;
  if (ctx->src.dirty) rc = cov_prep_async(ctx, false);
  return rc;
}

// Upload strided host records (or copy device records) and pack to float4 (original order).
int mgicp::upload_cloud(mgicp_ctx* ctx, Cloud& cl, const float* xyz, size_t n, size_t stride,
                 bool device_ptr) {
  if (n == 0 || !xyz || stride < 12 || (stride % 4) != 0)
    return fail(ctx, MGICP_E_INVALID, "invalid cloud (null, empty or stride not a multiple of 4 >= 12)");
  if (n >= (size_t(1) << 31) - 1)  // 32-bit point indices / hipcub item counts
    return fail(ctx, MGICP_E_INVALID, "cloud too large: at most 2^31 - 2 points per cloud");
  if (&cl == &ctx->tgt || &cl == &ctx->src) {  // an async covariance launch still reads the old cloud
    const int rj = cov_join(ctx, &cl == &ctx->tgt);
    if (rj) return rj;
  }
  if (&cl == &ctx->src && ctx->qperm_aux)  // the aux stream's Morton sort still reads the source's grid
    HIPCK(hipStreamWaitEvent(ctx->stream, ctx->aux_ev[2], 0));
  const double t0 = now_ms();
  MGICP_TRACE_AT("upload: begin");
  HIPCK(cl.orig.reserve(n));
  MGICP_TRACE_AT("upload: orig reserved");
  if (device_ptr) {
    HIPCK(launch_pack_points(xyz, n, stride, cl.orig.p, ctx->stream));
  } else {
    // host workers pack xyz into pinned slots while earlier slots are in flight
    HostUploader& up = HostUploader::instance();
    HIPCK(up.init(ctx->host_threads));
    HIPCK(ctx->xyz_dev.reserve(3 * n));
    MGICP_TRACE_AT("upload: staging ready");
    {
      std::lock_guard<std::mutex> lk(up.mu);
      HIPCK(upload_xyz(*up.pool, up.ring, xyz, n, stride, ctx->xyz_dev.p, ctx->stream));
    }
    MGICP_TRACE_AT("upload: all chunks queued");
    HIPCK(launch_pack_points(ctx->xyz_dev.p, n, 12, cl.orig.p, ctx->stream));
  }
  int rc = sync(ctx);
  if (rc) return rc;
  MGICP_TRACE_AT("upload: synced");
  cl.n = n;
  cl.dirty = true;
  cl.have_cov = false;
  if (&cl == &ctx->src) ctx->qperm_valid = false;
  if (&cl == &ctx->src || &cl == &ctx->tgt) {
    // the previous sweep's matches index the old clouds: never seed from / reuse them
    ctx->have_corr = false;
    ctx->seed_valid = false;
    ctx->ms_upload_pending += now_ms() - t0;
  }
  return MGICP_OK;
}

// r05 target cache.  A single-rank context leaves its target at destroy when the grid is the one a fresh
// context would build for those points (fresh_grid; since r06 every grid is sized from its own cloud
// alone -- DESIGN.md "Target cache").
void mgicp::tcache_donate(mgicp_ctx* ctx, bool cov_complete) {
  Cloud& t = ctx->tgt;
  if (!ctx->tcache_on || ctx->nranks != 1 || ctx->comm || ctx->have_shm || t.dirty || t.n == 0 || t.n_built != t.n ||
      !t.fresh_grid)
    return;
  TargetCache& c = g_tcache[ctx->device & 63];
  std::lock_guard<std::mutex> lk(c.mu);
  tcache_clear_locked(c);
  swap_target_state(c.t, t);
  c.t.n = t.n;
  c.t.have_cov = cov_complete && (!t.have_cov || (t.cov_p0 == 0 && t.cov_p1 == t.n)) && c.t.cov_stride == t.n;
  c.t.cov_p0 = 0;
  c.t.cov_p1 = t.n;
  c.t.want_empty_map = t.want_empty_map;
  c.t.want_seed_map = t.want_seed_map;
  c.t.drop_nonfinite = t.drop_nonfinite;
  c.t.fresh_grid = true;
  c.k = ctx->prm.k;
  c.eps = ctx->prm.gicp_eps;
  // the cell lists travel with the target once built (the donor ran 3+ aligns on it).  The list policy
  // itself does not go on across contexts: GICPState's engines run 2 aligns each, and building the lists
  // in a later cycle cost 39 + 151 ms at C4 (profiles/r05/check5) against ~1.6 ms saved per cycle
  // (not from a context with a test-sized pool, debug option "vlist_pool": an adopter would inherit its cap)
  c.vl_valid = ctx->vl_valid && ctx->vl_alloc && ctx->vl_pool_entries == 0;
  if (c.vl_valid) swap_list_state(c, *ctx);
  c.valid = true;
  c.donations++;
}

// After set_target's upload: the cached state when the uploaded points equal the cached ones bit for bit
// (original order, w = original index).  The context's previous target buffers go to its graveyard.
int mgicp::tcache_adopt(mgicp_ctx* ctx) {
  ctx->tcache_adopted = false;
  Cloud& t = ctx->tgt;
  if (!ctx->tcache_on || ctx->nranks != 1 || ctx->comm || ctx->have_shm) return MGICP_OK;
  TargetCache& c = g_tcache[ctx->device & 63];
  std::lock_guard<std::mutex> lk(c.mu);
  if (!c.valid || c.t.n != t.n || c.t.drop_nonfinite != t.drop_nonfinite)
    return MGICP_OK;
  unsigned int* diff = reinterpret_cast<unsigned int*>(ctx->d_small);
  MGICP_TRACE_AT("adopt: compare");
  HIPCK(launch_equal(t.orig.p, c.t.orig.p, t.n, diff, ctx->stream));
  int rc = sync(ctx);
  if (rc) return rc;
  MGICP_TRACE_AT("adopt: compared");
  unsigned int d = 1;
  std::memcpy(&d, ctx->h_small, sizeof(d));
  if (d != 0) return MGICP_OK;
  swap_target_state(t, c.t);
  t.dirty = false;
  t.have_cov = c.t.have_cov && c.k == ctx->prm.k && c.eps == ctx->prm.gicp_eps;
  t.cov_p0 = 0;
  t.cov_p1 = t.have_cov ? t.n : 0;
  t.fresh_grid = true;
  ctx->vl_valid = c.vl_valid;
  if (c.vl_valid) swap_list_state(*ctx, c);
  // the cache now holds this context's previous target buffers: to the graveyard (freed at a quiet point)
  Cloud none;
  each_target_buf(c.t, none, [&](auto& x, auto&) {
    if (x.p) ctx->grave->v.push_back(x.p);
    x.p = nullptr;
    x.cap = 0;
  });
  for (void* p : {static_cast<void*>(c.vl_cell.p), static_cast<void*>(c.vl_pool.p), static_cast<void*>(c.vl_ctr.p)})
    if (p) ctx->grave->v.push_back(p);
  c.vl_cell.p = nullptr; c.vl_cell.cap = 0;
  c.vl_pool.p = nullptr; c.vl_pool.cap = 0;
  c.vl_ctr.p = nullptr; c.vl_ctr.cap = 0;
  c.valid = false;
  c.hits++;
  ctx->tcache_adopted = true;
  return MGICP_OK;
}

// Bounding box of n points, folded on the host: the kernel's block partials (8 floats each: min, max,
// the block's non-finite count) land straight in mapped host memory (nb * 8 floats <= 32 KiB): no copy.
// bad (nullable): the non-finite points; queued (nullable): the trace label between launch and drain.
int mgicp::bbox_to_host(mgicp_ctx* ctx, const float4* pts, size_t n, float lo[3], float hi[3], double* bad,
                        const char* queued) {
  const int nb = static_cast<int>(std::min<size_t>((n + 255) / 256, 1024));
  HIPCK(launch_bbox(pts, n, reinterpret_cast<float*>(ctx->d_small), nb, ctx->stream));
  if (queued) MGICP_TRACE_AT(queued);
  int rc = sync(ctx);
  if (rc) return rc;
  const float* hp = reinterpret_cast<const float*>(ctx->h_small);
  double nbad = 0;
  for (int d = 0; d < 3; ++d) {
    lo[d] = INFINITY;
    hi[d] = -INFINITY;
  }
  for (int b = 0; b < nb; ++b) {
    for (int d = 0; d < 3; ++d) {
      lo[d] = std::min(lo[d], hp[b * 8 + d]);
      hi[d] = std::max(hi[d], hp[b * 8 + 3 + d]);
    }
    nbad += hp[b * 8 + 6];
  }
  if (bad) *bad = nbad;
  return MGICP_OK;
}

// Build the row-sorted uniform grid of a cloud (one-time per set_*).
int mgicp::build_grid(mgicp_ctx* ctx, Cloud& cl, bool defer_extras) {
  const size_t n = cl.n;
  hipStream_t s = ctx->stream;
  // 1. bounding box + finiteness
  MGICP_TRACE_AT("grid: begin");
  float mn[3], mx[3];
  double bad = 0;
  int rc = bbox_to_host(ctx, cl.orig.p, n, mn, mx, &bad, "grid: bbox queued");
  if (rc) return rc;
  MGICP_TRACE_AT("grid: bbox synced");
  if (bad > 0 && cl.drop_nonfinite) {
    // keep the finite points (original indices stay in w) and rebuild from them
    HIPCK(ctx->f_flags.reserve(n + 1));
    HIPCK(ctx->f_pos.reserve(n + 1));
    HIPCK(cl.pts.reserve(n));
    const size_t sb = scan_scratch_bytes(n + 1);
    HIPCK(ctx->scratch.reserve(sb));
    HIPCK(launch_finite_compact(cl.orig.p, n, ctx->f_flags.p, ctx->f_pos.p, ctx->scratch.p, sb, cl.pts.p, s));
    HIPCK(hipMemcpyAsync(ctx->h_small, ctx->f_pos.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    uint32_t kept = 0;
    std::memcpy(&kept, ctx->h_small, sizeof(kept));
    if (kept > 0) HIPCK(hipMemcpyAsync(cl.orig.p, cl.pts.p, kept * sizeof(float4), hipMemcpyDeviceToDevice, s));
    cl.n = kept;
    if (kept == 0) {
      cl.dirty = false;
      return MGICP_OK;  // empty cloud: callers check cl.n
    }
    return build_grid(ctx, cl, defer_extras);
  }
  if (bad > 0) return fail(ctx, MGICP_E_NONFINITE, "cloud contains NaN/Inf coordinates");
  for (int d = 0; d < 3; ++d) {
    cl.lo[d] = mn[d];
    cl.hi[d] = mx[d];
  }
  float ext[3];
  float maxext = 0.f, maxabs = 0.f;
  for (int d = 0; d < 3; ++d) {
    ext[d] = mx[d] - mn[d];
    maxext = std::max(maxext, ext[d]);
    maxabs = std::max(maxabs, std::max(std::fabs(mn[d]), std::fabs(mx[d])));
  }
  // 2. cell size: aim at `target_occ` points per non-empty cell
  const double target_occ = kDefaultOccupancy;
  auto dims = [&](double h, int* nd) {
    size_t nc = 1;
    for (int d = 0; d < 3; ++d) {
      const float inv_h = static_cast<float>(1.0 / h);
      nd[d] = static_cast<int>(std::floor(static_cast<double>(ext[d]) * inv_h)) + 1;
      nc *= static_cast<size_t>(nd[d]);
    }
    return nc;
  };
  double h = maxext > 0.f ? static_cast<double>(maxext) / std::cbrt(static_cast<double>(n)) : 1.0;
  // r06: the cell size is a function of this cloud alone -- never of this slot's
  // previous grid or of the other cloud's (the source's grid sets the order of every objective sum).
  // One sketch pass (cell_sketch_kernel) estimates the non-empty cells at kSketchScales sizes
  // h0 * 2^(k - 10) around the 3-D guess h0 above; the size is interpolated in log-log between the two
  // that bracket the target occupancy.  r01-r05 ran trial histograms instead (scattered atomics, a host
  // round trip each, two per cloud on a surface: ~0.6-0.8 ms per 5M cloud before the sort)
  const bool fresh = true;
  h = std::max(h, 1e-6);
  if (cl.force_h > 0) {
    // the caller's cell edge (Euclidean clustering: tolerance / 2), no sketch; at most 2^20 cells per axis
    // (bcell's clamp), the dense-table cap below may still grow it
    h = std::max(cl.force_h, static_cast<double>(maxext) / 1048576.0);
  } else if (maxext > 0.f && n > 1) {
    SketchScales sc;
    double hk[kSketchScales];
    for (int k = 0; k < kSketchScales; ++k) {
      hk[k] = h * std::ldexp(1.0, k - 10);
      sc.inv[k] = static_cast<float>(1.0 / hk[k]);
    }
    HIPCK(ctx->scratch.reserve(static_cast<size_t>(kSketchBlocks + 32) * kSketchScales * kSketchR));
    HIPCK(launch_cell_sketch(cl.orig.p, n, mn[0], mn[1], mn[2], sc, ctx->scratch.p, ctx->d_small + kSketchOffset, s));
    rc = sync(ctx);
    if (rc) return rc;
    MGICP_TRACE_AT("grid: sizing sketch synced");
    const unsigned char* regs = ctx->h_small + kSketchOffset;
    double occ[kSketchScales];
    for (int k = 0; k < kSketchScales; ++k) {
      // HyperLogLog estimate of the non-empty cells (linear counting while registers are still zero)
      double inv_sum = 0.0;
      int zeros = 0;
      for (int j = 0; j < kSketchR; ++j) {
        const int r = regs[k * kSketchR + j];
        inv_sum += std::ldexp(1.0, -r);
        zeros += r == 0;
      }
      const double R = kSketchR;
      double e = 0.7213 / (1.0 + 1.079 / R) * R * R / inv_sum;
      if (e <= 2.5 * R && zeros > 0) e = R * std::log(R / zeros);
      occ[k] = static_cast<double>(n) / std::max(e, 1.0);
    }
    int k1 = -1;
    for (int k = 0; k < kSketchScales && k1 < 0; ++k)
      if (occ[k] >= target_occ) k1 = k;
    if (k1 < 0) {
      h = hk[kSketchScales - 1];  // fewer points than the target per cell even at the coarsest size
    } else if (k1 == 0) {
      // finer than the finest size: extrapolate with the finest pair's growth exponent (1-3)
      double dim = std::log(std::max(occ[1], occ[0]) / occ[0]) / std::log(2.0);
      dim = std::min(3.0, std::max(1.0, dim));
      h = hk[0] * std::pow(target_occ / occ[0], 1.0 / dim);
    } else {
      const double t = (std::log(target_occ) - std::log(occ[k1 - 1])) / (std::log(occ[k1]) - std::log(occ[k1 - 1]));
      h = hk[k1 - 1] * std::exp2(std::min(1.0, std::max(0.0, t)));
    }
    h = std::max(h, 1e-6);
    if (trace_on()) {
      std::fprintf(stderr, "[mgicp] grid sizing n %zu h0 %.6g -> h %.6g (target %.1f); estimated occupancy", n, hk[10],
                   h, target_occ);
      for (int k = 0; k < kSketchScales; ++k) std::fprintf(stderr, " %.3g", occ[k]);
      std::fprintf(stderr, "\n");
    }
  }
  int nd[3];
  size_t nc = dims(h, nd);
  while (nc > kMaxCells) {
    h *= std::cbrt(static_cast<double>(nc) / kMaxCells) * 1.01;
    nc = dims(h, nd);
  }
  const float inv_h = static_cast<float>(1.0 / h);
  // 3. cell keys, stable radix sort -> permutation, cell_start from the sorted keys (cell_end_kernel +
  // an exclusive max-scan: no histogram of atomics)
  HIPCK(ctx->counts.reserve(nc + 1));
  HIPCK(ctx->keys.reserve(n));
  HIPCK(ctx->keys_sorted.reserve(n));
  HIPCK(ctx->vals.reserve(n));
  HIPCK(cl.perm.reserve(n));
  HIPCK(cl.cell_start.reserve(nc + 1));
  HIPCK(cl.pts.reserve(n));
  MGICP_TRACE_AT("grid: final buffers reserved");
  HIPCK(launch_cell_keys(cl.orig.p, n, mn[0], mn[1], mn[2], inv_h, nd[0], nd[1], nd[2], ctx->keys.p, s));
  int bits = 1;
  while ((size_t(1) << bits) < nc && bits < 32) ++bits;
  const size_t sb = std::max(sort_scratch_bytes(n, bits), cell_start_scratch_bytes(nc));
  HIPCK(ctx->scratch.reserve(sb));
  HIPCK(launch_iota(ctx->vals.p, n, s));
  HIPCK(launch_sort_pairs(ctx->scratch.p, sb, ctx->keys.p, ctx->keys_sorted.p, ctx->vals.p,
                          cl.perm.p, n, bits, s));
  HIPCK(launch_cell_starts(ctx->keys_sorted.p, n, nc, ctx->counts.p, cl.cell_start.p, ctx->scratch.p, sb, s));
  HIPCK(launch_gather_sorted(cl.orig.p, cl.perm.p, n, cl.pts.p, s));
  MGICP_TRACE_AT("grid: sort queued");
  if (trace_on() && n > 0) {  // diagnostics: the grid's real occupancy (host copy of the sorted keys)
    std::vector<uint32_t> ks(n);
    HIPCK(hipMemcpyAsync(ks.data(), ctx->keys_sorted.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    size_t runs = 1;
    for (size_t i = 1; i < n; ++i) runs += ks[i] != ks[i - 1];
    std::fprintf(stderr, "[mgicp] grid n %zu h %.6g cells %d x %d x %d, non-empty %zu, occupancy %.2f\n", n, h, nd[0],
                 nd[1], nd[2], runs, static_cast<double>(n) / runs);
  }
  if (!defer_extras) {
    rc = sync(ctx);
    if (rc) return rc;
    MGICP_TRACE_AT("grid: sorted");
  }
  // the build scratch stays allocated for the next build (hipFree + hipMalloc of these
  // tens-of-MB buffers cost milliseconds of host time between the two clouds' builds)
  GridView& g = cl.view;
  g.ox = mn[0];
  g.oy = mn[1];
  g.oz = mn[2];
  g.h = static_cast<float>(h);
  g.inv_h = inv_h;
  // rounding slack: a few ulps of the largest coordinate plus a sliver of a cell
  g.slop = 8.f * maxabs * 1.1920929e-7f + 1e-6f * static_cast<float>(h);
  g.nx = nd[0];
  g.ny = nd[1];
  g.nz = nd[2];
  g.cell_start = cl.cell_start.p;
  g.pts = cl.pts.p;
  g.empty_dist = nullptr;
  g.seed = nullptr;
  g.pairs = nullptr;
  cl.ncells = nc;
  cl.n_built = n;
  cl.fresh_grid = fresh;
  cl.dirty = false;
  cl.have_cov = false;
  if (&cl == &ctx->tgt) ctx->vl_valid = false;  // the 1-NN cell lists index the old target
  if (&cl == &ctx->src) ctx->src_lazy_ready = false;  // lazy covariances: none computed for this cloud
  if (&cl == &ctx->src || &cl == &ctx->tgt) {  // sorted positions changed
    ctx->have_corr = false;
    ctx->seed_valid = false;
  }
  return defer_extras ? MGICP_OK : build_grid_extras(ctx, cl);
}

// Upload a cloud into ctx->aux and build its grid over the finite points (the reference's KdTreeFLANN
// holds only those); force_h > 0: with that cell edge.  Both flags are the call's own and are back at
// their defaults on every return.  An empty grid (no finite point) is not an error: callers check aux.n.
int mgicp::aux_grid(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, double force_h) {
  int rc = upload_cloud(ctx, ctx->aux, xyz, n, stride, false);
  if (rc) return rc;
  ctx->aux.drop_nonfinite = true;
  ctx->aux.force_h = force_h;
  rc = build_grid(ctx, ctx->aux);
  ctx->aux.drop_nonfinite = false;
  ctx->aux.force_h = 0.0;
  return rc;
}

// query order of the shard's 1-NN sweeps and source covariances (once per source cloud and shard)
const uint32_t* mgicp::query_perm(mgicp_ctx* ctx) {
  if (ctx->qperm_aux) {  // sorted on the aux stream at set_source: the main stream waits for it on the device
    ctx->qperm_aux = false;
    if (hipStreamWaitEvent(ctx->stream, ctx->aux_ev[2], 0) != hipSuccess) ctx->qperm_valid = false;
  }
  if (ctx->qperm_valid) return ctx->qperm.p;
  const size_t p0 = ctx->shard_p0(), ns = ctx->shard_p1() - p0;
  if (ns == 0 || !morton_perm(ctx, ctx->src, p0, ns, ctx->qperm, false)) return nullptr;
  ctx->qperm_valid = true;
  return ctx->qperm.p;
}

// covariances of sorted positions [p0, p1) into arrays of `stride` entries (default n)
int mgicp::compute_cov(mgicp_ctx* ctx, Cloud& cl, size_t p0, size_t p1, size_t stride) {
  MGICP_TRACE_AT("cov: begin");
  if (stride < cl.n) stride = cl.n;
  HIPCK(cl.cov.reserve(3 * stride));
  cl.cov_stride = stride;
  MGICP_TRACE_AT("cov: reserved");
  // grid order, not Morton order: the k = 20 queries sit on the surface and the row-major order
  // measured faster (3.97 vs 4.42 ms at 5M, profiles/r01/ab_qorder/)
  const uint32_t* perm = nullptr;
  const bool logged = ctx->knn_logged;
  if (logged) {
    HIPCK(ctx->knn_fb.reserve(p1 - p0));
    HIPCK(ctx->u64.reserve(1));
    HIPCK(hipMemsetAsync(ctx->u64.p, 0, sizeof(unsigned long long), ctx->stream));
  }
  unsigned int* fb_count = reinterpret_cast<unsigned int*>(ctx->u64.p);
  {
    ProfScope ps(ctx, kFamCov);
    HIPCK(launch_knn_cov(cl.view, ctx->prm.k, ctx->prm.gicp_eps, p0, p1, cl.cov3(), perm,
                         logged ? ctx->knn_fb.p : nullptr, logged ? fb_count : nullptr, ctx->stream));
  }
  if (logged) {
    // the points the logged kernel left to the register-list kernel (log overflow, ties at tau)
    HIPCK(hipMemcpyAsync(ctx->h_small, fb_count, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    int rc0 = sync(ctx);
    if (rc0) return rc0;
    unsigned int nfb = 0;
    std::memcpy(&nfb, ctx->h_small, sizeof(nfb));
    ctx->knn_fallbacks = nfb;
    const bool stats = knn_stats_on();
    if (stats) std::fprintf(stderr, "[knn] %zu points, %u left to the register-list kernel\n", p1 - p0, nfb);
    if (nfb) {
      ProfScope ps(ctx, kFamCov);
      if (ctx->knn_wave && nfb <= kWaveKnnMax)
        HIPCK(launch_knn_wave(cl.view, ctx->prm.k, ctx->prm.gicp_eps, ctx->knn_fb.p, nullptr, nfb, cl.cov3(), ctx->stream));
      else
        HIPCK(launch_knn_cov(cl.view, ctx->prm.k, ctx->prm.gicp_eps, 0, nfb, cl.cov3(), ctx->knn_fb.p, nullptr,
                             nullptr, ctx->stream));
    }
  }
  int rc = sync(ctx);
  if (rc) return rc;
#if defined(MGICP_CORR_PHASES) && MGICP_CORR_PHASES
  {
    unsigned long long ph[24];
    HIPCK(corr_phase_take(ph));
    if (ph[0])
      std::fprintf(stderr, "[knnb] waves %llu staged %llu (non-monotone %llu, over the cap %llu) | per wave: union points %.1f, "
                   "pieces %.1f, block candidates mean lane %.1f busiest lane %.1f | lanes past the block %llu, hand-offs %llu "
                   "of %llu\n", ph[0], ph[1], ph[4], ph[5], double(ph[2]) / ph[0], double(ph[3]) / ph[0],
                   double(ph[6]) / ph[0] / 64.0, double(ph[7]) / ph[0], ph[8], ph[9], ph[10]);
    if (ph[0] && ph[1] && ph[0] > ph[1])
      std::fprintf(stderr, "[knnb] cycles per wave -- staged: setup %.0f, copy %.0f, passes %.0f | unstaged: setup %.0f, "
                   "passes %.0f\n", double(ph[11]) / ph[1], double(ph[12]) / ph[1], double(ph[13]) / ph[1],
                   double(ph[15]) / (ph[0] - ph[1]), double(ph[16]) / (ph[0] - ph[1]));
    const double w = ph[21] ? static_cast<double>(ph[21]) : 1.0;
    std::fprintf(stderr, "[knn-div] waves %llu | per wave: test iterations %.1f, max lane tests %.1f, mean lane tests %.1f"
                 " | cycles/wave search %.0f, moments + finish %.0f\n",
                 ph[21], ph[18] / w, ph[19] / w, ph[20] / w / 64.0, ph[22] / w, ph[23] / w);
  }
#endif
  MGICP_TRACE_AT("cov: done");
  cl.have_cov = true;
  cl.cov_p0 = p0;
  cl.cov_p1 = p1;
  return MGICP_OK;
}

// target covariances (computeCovariances on the target, once per target cloud).  Multi-GPU
// (SURVEY.md 8e): rank r computes the r-th of N equal slices and one in-place all-gather per
// covariance array (48 bytes per point in total) completes every rank's copy -- the values are
// per point, so the result is the single-GPU one bit for bit.
int mgicp::target_cov(mgicp_ctx* ctx) {
  Cloud& t = ctx->tgt;
  if (!ctx->comm || ctx->nranks < 2) return compute_cov(ctx, t, 0, t.n);
  const size_t N = static_cast<size_t>(ctx->nranks), r = static_cast<size_t>(ctx->rank);
  const size_t cnt = (t.n + N - 1) / N;
  int rc = compute_cov(ctx, t, std::min(t.n, r * cnt), std::min(t.n, (r + 1) * cnt), N * cnt);
  if (rc) return rc;
  const Cov3 c = t.cov3();
  NCCLCK(ncclGroupStart());
  for (double2* a : {c.a, c.b, c.c})
    NCCLCK(ncclAllGather(a + r * cnt, a, 2 * cnt, ncclDouble, ctx->comm, ctx->stream));
  NCCLCK(ncclGroupEnd());
  if ((rc = sync(ctx))) return rc;
  t.cov_p0 = 0;
  t.cov_p1 = t.n;
  return MGICP_OK;
}

// the covariances a sweep needs (lazy source mode): its accepted source points without one, computed
// by the same kernels as the eager pass (the k-NN kernel, the register-list hand-off for the rest)
int mgicp::cov_lazy(mgicp_ctx* ctx) {
  if (!ctx->lazy_src_cov || ctx->src.have_cov) return MGICP_OK;
  const size_t p0 = ctx->shard_p0(), ns = ctx->shard_p1() - p0;
  HIPCK(ctx->u64.reserve(1));
  unsigned int* cnt = reinterpret_cast<unsigned int*>(ctx->u64.p);  // [0] points to compute, [1] hand-offs
  HIPCK(hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned int), ctx->stream));
  HIPCK(launch_cov_need(ctx->flags.p, ctx->cov_ok.p, p0, ns, ctx->cov_need.p, cnt, ctx->stream));
  HIPCK(hipMemcpyAsync(ctx->h_small, cnt, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
  int rc = sync(ctx);
  if (rc) return rc;
  unsigned int need = 0;
  std::memcpy(&need, ctx->h_small, sizeof(need));
  if (knn_stats_on()) std::fprintf(stderr, "[knn-lazy] source covariances to compute for this sweep: %u\n", need);
  if (!need) return MGICP_OK;
  // r06: few points (after the head start: mostly the isolated ones its ring cap left -- C4F's debris and
  // clutter near the part, 21k in the first sweep) run one wave each, so their long ring searches do not
  // leave a few per-lane waves as the launch's tail (C4F: 5 ms -> 0.9 ms); a bulk list (the synchronous
  // path -- N > 1 ranks, profiling -- where the first sweep needs every source covariance) keeps the
  // per-lane kernels, 64 points per wave
  if (ctx->knn_wave && need <= kWaveKnnMax) {
    ProfScope ps(ctx, kFamCov);
    HIPCK(launch_knn_wave(ctx->src.view, ctx->prm.k, ctx->prm.gicp_eps, ctx->cov_need.p, nullptr, need, ctx->src.cov3(),
                          ctx->stream));
    return MGICP_OK;
  }
  const bool logged = ctx->knn_logged;
  if (logged) HIPCK(ctx->knn_fb.reserve(need));
  {
    ProfScope ps(ctx, kFamCov);
    HIPCK(launch_knn_cov(ctx->src.view, ctx->prm.k, ctx->prm.gicp_eps, 0, need, ctx->src.cov3(), ctx->cov_need.p,
                         logged ? ctx->knn_fb.p : nullptr, logged ? cnt + 1 : nullptr, ctx->stream));
  }
  if (logged) {
    HIPCK(hipMemcpyAsync(ctx->h_small, cnt + 1, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    unsigned int nfb = 0;
    std::memcpy(&nfb, ctx->h_small, sizeof(nfb));
    ctx->knn_fallbacks = nfb;
    ProfScope ps(ctx, kFamCov);
    if (nfb)
      HIPCK(launch_knn_cov(ctx->src.view, ctx->prm.k, ctx->prm.gicp_eps, 0, nfb, ctx->src.cov3(), ctx->knn_fb.p, nullptr,
                           nullptr, ctx->stream));
  }
  return MGICP_OK;
}

extern "C" {

void mgicp_release_cache(void) {
  int dev = 0;
  const bool have = hipGetDevice(&dev) == hipSuccess;
  for (int d = 0; d < 64; ++d) {
    TargetCache& c = g_tcache[d];
    std::lock_guard<std::mutex> lk(c.mu);
    if (!c.valid && !c.t.orig.p && !c.vl_pool.p) continue;
    (void)hipSetDevice(d);
    tcache_clear_locked(c);
  }
  if (have) (void)hipSetDevice(dev);
}

}  // extern "C"
