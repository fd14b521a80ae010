// mgicp_engine.hip -- host engine behind include/mi355x_gicp.h (libmgicp.so).
//
// Replaces pcl::GeneralizedIterativeClosestPoint<PointXYZRGB,PointXYZRGB>::align as called
// at the reference's src/GICPAlignment.cpp:96 (and :116 via iterate()).  The outer loop is
// GICP::computeTransformation (registration/impl/gicp.hpp): per iteration one correspondence
// sweep on the GPU, then estimateRigidTransformationBFGS whose objective passes run on the
// GPU and whose 6-DoF BFGS logic runs here (pcl_bfgs.hpp), then PCL's delta test.
// Multi-GPU: one process per GPU, contiguous ranges of the grid-sorted source cloud per rank,
// target replicated; the per-pass sums travel through a node-wide shared-memory segment of super
// rows (shm_rows.hpp: every rank's GPU writes its rows, every host takes the same fixed-order
// total), or -- without that segment -- one RCCL all-gather of super partials per pass (xGMI).
// This file: the context's life, the sweeps, the two solvers' outer steps and mgicp_align.  The clouds
// and their grids / covariances are in mgicp_clouds.hip, the objective passes in mgicp_pass.hip, the
// transports in mgicp_comm.hip, the calls beside the alignment in mgicp_fod.hip and mgicp_features.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "host_upload.hpp"
#include "mgicp_ctx.hpp"
#include "gn_solver.hpp"

using namespace mgicp;

thread_local Graveyard* mgicp::t_new_ctx_grave = nullptr;

namespace {

constexpr size_t kSmallBytes = size_t(64) << 10;  // pinned readback scratch per context

// transform_R(i,j) = sum_k double(T(i,k)) * double(G(k,j)), top-left 3x3
Rot33d rot_of(const Mat4& T, const Mat4& G) {
  Rot33d R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double a = 0.0;
      for (int k = 0; k < 4; ++k) a += static_cast<double>(T.m[i][k]) * static_cast<double>(G.m[k][j]);
      R.m[3 * i + j] = a;
    }
  return R;
}

// The fine grid of the target's 1-NN cell lists for the current gate (once per target grid and gate;
// the lists themselves are built by the sweeps, cell by cell, the first time a query lands in a cell).
// The grid covers the target's bbox grown by the gate + 2 cells, so a query outside it is farther than
// the gate from every target point; cells of kVlistCell x the target grid's cell edge, fewer than 2^28
// cells (else the lists are off for this gate: the r03 sweeps).
constexpr double kVlistCell = 0.6f;  // fine cell edge / the target grid's cell edge (the float 0.6f, widened)
int vl_prepare(mgicp_ctx* ctx) {
  const double gate = ctx->prm.max_corr_dist;
  const size_t ns = ctx->shard_p1() - ctx->shard_p0();
  if (!(ctx->vl_valid && ctx->vl.gate == gate)) {
    ctx->vl_valid = false;
    ctx->vl_off = false;
    const Cloud& t = ctx->tgt;
    const double h = t.view.h;
    double c = std::max(h * kVlistCell, 1e-6);
    double ext = 0, maxabs = 0;
    for (int d = 0; d < 3; ++d) {
      ext = std::max(ext, static_cast<double>(t.hi[d] - t.lo[d]));
      maxabs = std::max(maxabs, std::max(std::fabs(static_cast<double>(t.lo[d])), std::fabs(static_cast<double>(t.hi[d]))));
    }
    constexpr size_t kVlMaxCells = size_t(1) << 28;
    int nd[3] = {0, 0, 0};
    double pad = 0;
    // (the cell counts in double: PCL's default gate, sqrt(DBL_MAX), is far outside an int or a size_t;
    // such a gate leaves the loop with c past 4 h, or not a number, and the lists are off)
    const double c_max = 4.0 * std::max(h, 1e-6);
    for (int it = 0; it < 64 && c <= c_max; ++it) {
      pad = gate * (1.0 + 1e-5) + 1e-9 + 2.0 * c;
      double nc = 1.0;
      for (int d = 0; d < 3; ++d) {
        const double m = std::floor((static_cast<double>(t.hi[d] - t.lo[d]) + 2.0 * pad) / c) + 1.0;
        nd[d] = m < 2147483647.0 ? static_cast<int>(m) : 2147483647;
        nc *= m;
      }
      if (nc <= static_cast<double>(kVlMaxCells)) break;
      c *= std::cbrt(nc / static_cast<double>(kVlMaxCells)) * 1.01;
    }
    ctx->vl.gate = gate;
    if (!(c <= c_max)) {  // a gate this wide against this target: lists would overflow
      ctx->vl_off = true;
      ctx->vl_valid = true;
      return MGICP_OK;
    }
    const size_t nc = static_cast<size_t>(nd[0]) * nd[1] * nd[2];
    VListView& v = ctx->vl;
    v.ox = static_cast<float>(t.lo[0] - pad);
    v.oy = static_cast<float>(t.lo[1] - pad);
    v.oz = static_cast<float>(t.lo[2] - pad);
    v.c = static_cast<float>(c);
    v.inv_c = static_cast<float>(1.0 / c);
    // the fp32 cell assignment floor((q - o) * inv_c) of a query: a few ulps of the coordinates
    // and of the cell count, covered with a wide margin
    v.es = static_cast<float>(3.0e-6 * (maxabs + pad + ext) + 1e-4 * c);
    v.nx = nd[0];
    v.ny = nd[1];
    v.nz = nd[2];
    ctx->vl_ncells = nc;
    ctx->vl_valid = true;
    ctx->vl_alloc = false;
    ctx->vl_epoch = 0;
    ctx->vl_groups = 0;
  }
  // the state words and the pool (~0.4 + 2 GB at C4) only once a sweep uses the lists: the first align
  // after a set_target runs the r03 sweep and must not pay for their allocation (r04)
  if (!ctx->vl_off && !ctx->vl_alloc && ctx->vl_groups >= ctx->vl_cold_groups) {
    const Cloud& t = ctx->tgt;
    VListView& v = ctx->vl;
    const size_t nc = ctx->vl_ncells;
    HIPCK(ctx->vl_cell.reserve(nc));
    HIPCK(hipMemsetAsync(ctx->vl_cell.p, 0xff, nc * sizeof(uint32_t), ctx->stream));
    // list starts are stored in units of 4 entries in 25 bits: at most 2^27 entries (16 bytes each)
    // (debug option "vlist_pool": a small pool, so that tests reach the pool-full branch of the build)
    const size_t want = ctx->vl_pool_entries ? std::max<size_t>(ctx->vl_pool_entries, 4096)
                                             : std::max<size_t>(size_t(1) << 22, 32 * t.n);
    const size_t cap = std::min<size_t>(size_t(1) << 27, want);
    HIPCK(ctx->vl_pool.reserve(cap));
    HIPCK(ctx->vl_ctr.reserve(8));  // [4]: the build's second-pass cells (r06)
    HIPCK(hipMemsetAsync(ctx->vl_ctr.p, 0, 8 * sizeof(unsigned int), ctx->stream));
    v.cell = ctx->vl_cell.p;
    v.pool = ctx->vl_pool.p;
    v.pool_cap = static_cast<uint32_t>(cap);
    v.ctr = ctx->vl_ctr.p;
    ctx->vl_alloc = true;
  }
  if (ctx->vl_off || !ctx->vl_alloc) return MGICP_OK;
  // per-sweep lists sized by the shard (one request / pending entry per query at most)
  const size_t q = std::max<size_t>(ns, 1);
  HIPCK(ctx->vl_build.reserve(q));
  HIPCK(ctx->vl_bcentre.reserve(q));
  HIPCK(ctx->vl_pend.reserve(q));
  ctx->vl.build = ctx->vl_build.p;
  ctx->vl.bcentre = ctx->vl_bcentre.p;
  ctx->vl.build_cap = static_cast<uint32_t>(std::min(ctx->vl_build.cap, ctx->vl_ncells));
  ctx->vl.pend = ctx->vl_pend.p;
  if (++ctx->vl_epoch >= 0x40000000u) {  // epochs wrap: every touched mark then reads as "earlier sweep"
    ctx->vl_epoch = 1;
  }
  ctx->vl.epoch = ctx->vl_epoch;
  ctx->vl.eager = ctx->vl_eager ? 1 : 0;
  ctx->vl.tpts = ctx->tgt.pts.p;
  return MGICP_OK;
}

// The 1-NN sweep kernel of one correspondence phase: the target's cell lists (r04, default), else the
// wave-uniform scan (debug option "vlist" 0, and the first aligns after a set_target); exact, same
// results.
bool sweep_listed(const mgicp_ctx* ctx) {
  return ctx->vlist && ctx->vl_valid && ctx->vl_alloc && !ctx->vl_off && ctx->vl_groups >= ctx->vl_cold_groups;
}

// fc (nullable, listed sweeps only): the compaction fused into the sweep
hipError_t launch_sweep(mgicp_ctx* ctx, const Mat4& T, double thr, bool seeded, const uint32_t* qp,
                        const FusedCompact* fc = nullptr) {
  const size_t p0 = ctx->shard_p0(), p1 = ctx->shard_p1();
  const GridView& g = ctx->tgt.view;
  if (sweep_listed(ctx)) ctx->vl_ctr_zero = nullptr;  // this sweep fills the counters and may leave them non-zero
  if (sweep_listed(ctx))
    return launch_vl_sweep(g, ctx->vl, ctx->d_out, p0, p1, T.xf(), thr, seeded ? 1 : 0, ctx->prev_pos.p, ctx->flags.p,
                           ctx->cus, ctx->stream, fc);
  return launch_correspond_wave(g, ctx->d_out, p0, p1, T.xf(), thr, seeded ? 1 : 0, ctx->prev_pos.p, ctx->flags.p, qp,
                                ctx->stream);
}

// Diagnostics of the sweep just queued, on stderr: the cell lists' statistics (debug option
// "vlist_stats") and the device counters of the diagnostic builds (make variant, DEFS=-DMGICP_VL_DIAG=1 /
// -DMGICP_CORR_PHASES=1 / -DMGICP_CORR_STATS=1).  Each drains the stream; a product build with the
// option off does nothing here.
int report_sweep(mgicp_ctx* ctx) {
  hipStream_t s = ctx->stream;
  if (ctx->vl_stats && sweep_listed(ctx)) {
    unsigned int c3[3];
    HIPCK(hipMemcpyAsync(c3, ctx->vl_ctr.p, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    HIPCK(ctx->u64.reserve(64));
    HIPCK(launch_vl_stats(ctx->vl, ctx->vl_ncells, ctx->u64.p, s));
    unsigned long long st[64];
    HIPCK(hipMemcpyAsync(st, ctx->u64.p, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    double hist_mean = st[0] ? static_cast<double>(st[1]) / st[0] : 0.0;
    unsigned long long acc = 0, p95 = 0;
    for (int L = 0; L < 56; ++L) {
      acc += st[8 + L];
      if (!p95 && acc >= 0.95 * st[0]) p95 = L;
    }
    std::fprintf(stderr, "[vlist] cell %.3f mm grid %dx%dx%d | sweep: %u cells requested, %u queries pending | lists %llu "
                 "(mean %.1f, p95 %llu entries), reject %llu, overflow %llu, pool %u of %u\n",
                 1e3 * ctx->vl.c, ctx->vl.nx, ctx->vl.ny, ctx->vl.nz, c3[1], c3[2], st[0], hist_mean, p95, st[2], st[3],
                 c3[0], ctx->vl.pool_cap);
  }
#if defined(MGICP_VL_DIAG) && MGICP_VL_DIAG
  {
    unsigned long long ph[24];
    HIPCK(hipStreamSynchronize(s));
    HIPCK(corr_phase_take(ph));
    const double c = ph[0] ? static_cast<double>(ph[0]) : 1.0;
    if (ph[0] && sweep_listed(ctx))
      std::fprintf(stderr, "[vl-build] cells %llu | per cell: candidates %.1f, stage-1 survivors %.1f, kept %.1f | cycles/cell "
                   "gather %.0f, stage 1 %.0f, stage 2 %.0f | survivors <=8 %llu <=16 %llu <=32 %llu <=64 %llu <=128 %llu "
                   "<=256 %llu >256 %llu | stage-2 cycles of cells with > 64 survivors: %.1f %%\n",
                   ph[0], ph[1] / c, ph[2] / c, ph[3] / c, ph[4] / c, ph[5] / c, ph[6] / c, ph[9], ph[10], ph[11], ph[12],
                   ph[13], ph[14], ph[8], ph[6] ? 100.0 * ph[15] / ph[6] : 0.0);
  }
#elif defined(MGICP_CORR_PHASES) && MGICP_CORR_PHASES
  {
    unsigned long long ph[24];
    HIPCK(hipStreamSynchronize(s));
    HIPCK(corr_phase_take(ph));
    const double w = ph[7] ? static_cast<double>(ph[7]) : 1.0;
    std::fprintf(stderr, "[corr-phase] waves %llu (per-lane finish %llu) | cycles/wave seeds %.0f box %.0f scan %.0f "
                 "winner %.0f finish %.0f | waves by stragglers 0:%llu 1-4:%llu 5-16:%llu 17-63:%llu 64:%llu, "
                 "stragglers %llu | per-lane waves: none included %llu, rows %llu, x cells %llu, small balls %llu\n", ph[7],
                 ph[6], ph[0] / w, ph[1] / w, ph[2] / w, ph[3] / w, ph[4] / w, ph[8], ph[9], ph[10], ph[11], ph[12], ph[13],
                 ph[14], ph[15], ph[16], ph[17]);
  }
#endif
#if MGICP_CORR_STATS
  {
    unsigned long long st[8];
    HIPCK(hipStreamSynchronize(s));
    HIPCK(corr_stats_take(st));
    std::fprintf(stderr, "[corr-stats] wave scan: queries %llu accepted %llu rejected %llu | per-lane tests/query %.1f "
                 "ranges/query %.1f | lanes left to the per-lane search %llu | union-scan waves %llu of %llu, "
                 "candidates per union wave %.1f\n",
                 st[0], st[1], st[2], st[0] ? double(st[3]) / st[0] : 0.0, st[0] ? double(st[4]) / st[0] : 0.0, st[5],
                 st[7], (st[0] + 63) / 64, st[7] ? double(st[6]) / st[7] : 0.0);
  }
#endif
  return MGICP_OK;
}

// r08: the verdict of the fused listed sweep stamped `stamp` (vl_round_publish_kernel): spin on the three
// mapped words as wait_pass does on its completion word; after ~0.5 s fall back to a stream drain so a
// failed launch surfaces as an error instead of a hang.  c = ctr[1..3]: requested, pending, deferred.
int wait_round(mgicp_ctx* ctx, unsigned int stamp, unsigned int c[3]) {
  auto take = [&]() {
    for (int i = 0; i < 3; ++i) {
      const unsigned long long w = __atomic_load_n(ctx->h_round + i, __ATOMIC_ACQUIRE);
      if (static_cast<unsigned int>(w >> 32) != stamp) return false;
      c[i] = static_cast<unsigned int>(w);
    }
    return true;
  };
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    if (take()) return MGICP_OK;
    if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) break;
  }
  int rc = sync(ctx);
  if (rc) return rc;
  if (!take()) return fail(ctx, MGICP_E_HIP, "listed sweep finished without publishing its round counters");
  return MGICP_OK;
}

// every error return of an align (a HIP error mid-loop, MGICP_E_COMM from a quitting rank, ...) drains
// the stream and gives the device's server slot back, so other contexts on the device keep their
// resident server; the error message of the failure is kept
struct AlignDrain {
  mgicp_ctx* ctx;
  bool armed = true;
  ~AlignDrain() {
    if (!armed) return;
    const std::string err = ctx->err;
    cancel_gated(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    srv_release(ctx);
    if (!ctx->srv_ev.empty()) srv_resolve(ctx);
    ctx->err = err;
  }
};

// GICP::estimateRigidTransformationBFGS: 0 = accepted, MGICP_E_SOLVER = PCL would throw
int estimate_bfgs(mgicp_ctx* ctx, Mat4& T, int* n_corr) {
  GateGuard guard{ctx};
  Vec6 x;
  x[0] = T.m[0][3];
  x[1] = T.m[1][3];
  x[2] = T.m[2][3];
  x[3] = std::atan2(static_cast<double>(T.m[2][1]), static_cast<double>(T.m[2][2]));
  x[4] = std::asin(-static_cast<double>(T.m[2][0]));
  x[5] = std::atan2(static_cast<double>(T.m[1][0]), static_cast<double>(T.m[0][0]));
  DeviceFunctor fn{ctx};
  // the correspondence count arrives with the first objective pass (its count lane)
  double s[kRedVals];
  int rc = fn.pass(x, s);
  if (rc) return rc;
  *n_corr = static_cast<int>(s[13]);
  if (s[13] < 4) return MGICP_E_SOLVER;  // NotEnoughPointsException
  fn.memoise(x, s);  // seed the memo with this pass so minimizeInit reuses it
  fn.remember(x, s);  // and the run's table: the line search comes back to this transform
  PclBfgs<DeviceFunctor> bfgs(fn);
  const double gradient_tol = 1e-2;
  int inner = 0;
  int result = bfgs.init(x);
  result = kRunning;
  do {
    inner++;
    result = bfgs.step(x);
    if (bfgs.error) return bfgs.error;
    if (result) break;
    result = bfgs.test_gradient(gradient_tol);
  } while (result == kRunning && inner < ctx->prm.max_inner_iter);
  if (bfgs.error) return bfgs.error;
  if (result == kNoProgress || result == kSuccess || inner == ctx->prm.max_inner_iter) {
    T = apply_state(x);
    return MGICP_OK;
  }
  return MGICP_E_SOLVER;  // SolverDidntConvergeException
}

// the correspondence sweep of the Gauss-Newton mode: exact 1-NN (same kernel as the BFGS mode),
// then the moment pass; no scan / compaction (the moment pass reads the flags directly)
int correspond_gn(mgicp_ctx* ctx, const Mat4& T, const Mat4& G, bool seed) {
  const double thr = ctx->prm.max_corr_dist * ctx->prm.max_corr_dist;
  const bool seeded = seed && ctx->seed_valid;
  const uint32_t* qp = query_perm(ctx);
  if (ctx->vlist) {
    int rc = vl_prepare(ctx);
    if (rc) return rc;
  }
  {
    ProfScope ps(ctx, kFamCorr);
    HIPCK(launch_sweep(ctx, T, thr, seeded, qp));
  }
  ctx->seed_valid = true;
  ctx->have_corr = false;  // the SoA streams of the BFGS mode are not refreshed
  int rc = cov_join_all(ctx);
  if (rc) return rc;
  if ((rc = cov_lazy(ctx))) return rc;
  return moments_pass(ctx, T, G);
}

// Gauss-Newton estimate on the moments of the last sweep (taken at T); T <- solution.
// 0 = accepted, MGICP_E_SOLVER = fewer than 4 correspondences or a singular normal matrix.
int estimate_gn(mgicp_ctx* ctx, Mat4& T, int* n_corr) {
  *n_corr = static_cast<int>(ctx->mom[73]);
  if (ctx->mom[73] < 4) return MGICP_E_SOLVER;
  gn::Problem pb;
  pb.mom = ctx->mom;
  gn::Pose P;
  for (int a = 0; a < 3; ++a) {
    pb.c[a] = ctx->out_ctr[a];
    for (int k = 0; k < 4; ++k) pb.T0[a][k] = static_cast<double>(T.m[a][k]);
    for (int k = 0; k < 3; ++k) P.R[a][k] = pb.T0[a][k];
    P.t[a] = pb.T0[a][3];
  }
  int host_evals = 0;
  if (!gn::solve(pb, P, ctx->prm.max_inner_iter, &host_evals)) return MGICP_E_SOLVER;
  for (int a = 0; a < 3; ++a) {
    for (int k = 0; k < 3; ++k) T.m[a][k] = static_cast<float>(P.R[a][k]);
    T.m[a][3] = static_cast<float>(P.t[a]);
  }
  return MGICP_OK;
}

int check_params(mgicp_ctx* ctx, const mgicp_params& p) {
  if (p.k < 1 || p.k > kMaxK)
    return fail(ctx, MGICP_E_INVALID, "k (k_correspondences) must be in [1, 32]");
  // 0 is PCL's legal degenerate value; a NaN, negative or infinite one makes every covariance NaN or indefinite
  if (!(p.gicp_eps >= 0) || std::isinf(p.gicp_eps))
    return fail(ctx, MGICP_E_INVALID, "gicp_eps (gicp_epsilon) must be finite and >= 0");
  if (p.max_iter < 1 || p.max_inner_iter < 1 || !(p.max_corr_dist >= 0) || !(p.rot_eps > 0) ||
      !(p.tf_eps >= 0) ||
      (p.solver != MGICP_SOLVER_PCL_BFGS && p.solver != MGICP_SOLVER_GN))
    return fail(ctx, MGICP_E_INVALID, "invalid GICP parameters");
  return MGICP_OK;
}

// mgicp_set_{target,source}[_device]: the upload, the target cache's offer (target only), the head start
int set_cloud(mgicp_ctx* ctx, bool tgt, const float* xyz, size_t n, size_t stride, bool device_ptr) {
  if (!ctx) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = upload_cloud(ctx, tgt ? ctx->tgt : ctx->src, xyz, n, stride, device_ptr);
  if (!rc && tgt) rc = tcache_adopt(ctx);
  return rc ? rc : cov_prep_async_all(ctx);
}

// MGICP_PASS_DIAG builds (ensure_host_red allocates the timers there; null in a product build): the
// gated passes' and the resident server's per-pass times of the align just finished, on stderr
void report_pass_times(mgicp_ctx* ctx) {
  if (ctx->h_gtrace) {
    // diagnostics of the gated passes of this align: device-side gate wait and spread, host-side
    // decision time (sums seen -> command published); device wall clock in 10 ns ticks (100 MHz)
    double w = 0, sp = 0, hd = 0;
    int cnt = 0;
    for (int i = 0; i < 1024; ++i) {
      const unsigned long long* t = ctx->h_gtrace + 4 * i;
      if (!t[0] || !t[1] || !t[2] || ctx->host_gt[2 * i + 1] <= 0 || ctx->host_gt[2 * i] <= 0) continue;
      w += (t[1] - t[0]) * 0.01;
      sp += (static_cast<double>(t[2]) - static_cast<double>(t[1])) * 0.01;
      hd += ctx->host_gt[2 * i + 1] - ctx->host_gt[2 * i];
      ++cnt;
    }
    if (cnt)
      std::fprintf(stderr, "[gate-trace] passes %d | device: block-0 wait %.2f us, last block through the gate +%.2f us | host: sums seen -> command published %.2f us\n",
                   cnt, w / cnt, sp / cnt, hd / cnt);
    std::memset(ctx->h_gtrace, 0, 4 * 1024 * sizeof(unsigned long long));
    std::fill(ctx->host_gt.begin(), ctx->host_gt.end(), 0.0);
  }
  if (ctx->h_ptimes) {
    // diagnostics of the resident server: per pass, block 0's gate exit -> the finishing wave
    // (device active time) and the previous finish -> this gate exit (host turnaround + gate)
    double act = 0, gap = 0;
    int na = 0, ng = 0;
    for (int i = 0; i < 1024; ++i) {
      const unsigned long long* t = ctx->h_ptimes + 2 * i;
      if (t[0] && t[1] && t[1] > t[0]) { act += (t[1] - t[0]) * 0.01; ++na; }
      const unsigned long long* pv = ctx->h_ptimes + 2 * ((i + 1023) & 1023);
      if (t[0] && pv[1] && t[0] > pv[1] && t[0] - pv[1] < 100000) { gap += (t[0] - pv[1]) * 0.01; ++ng; }
    }
    if (na)
      std::fprintf(stderr, "[pass-times] passes %d | active %.2f us | finish -> next gate exit %.2f us (%d)\n", na,
                   act / na, ng ? gap / ng : 0.0, ng);
    if (ctx->ht_n)
      std::fprintf(stderr, "[pass-times] host view: %d passes | command -> rows complete %.2f us | rows -> next command %.2f us (BFGS step until the next pass %.2f us)\n",
                   ctx->ht_n, 1e3 * ctx->ht_dev / ctx->ht_n, ctx->ht_nh ? 1e3 * ctx->ht_host / ctx->ht_nh : 0.0,
                   ctx->ht_nh ? 1e3 * ctx->ht_bfgs / ctx->ht_nh : 0.0);
    if (ctx->ht_ne)
      std::fprintf(stderr, "[pass-times] host view: rows complete -> f, g of the pass ready %.2f us (%d)\n",
                   1e3 * ctx->ht_eval / ctx->ht_ne, ctx->ht_ne);
    ctx->ht_dev = ctx->ht_host = ctx->ht_bfgs = ctx->ht_eval = ctx->ht_last_rows = 0;
    ctx->ht_n = ctx->ht_nh = ctx->ht_ne = 0;
    std::memset(ctx->h_ptimes, 0, 2 * 1024 * sizeof(unsigned long long));
  }
}

}  // namespace

// Registration::initCompute + initComputeReciprocal + computeCovariances (both clouds)
int mgicp::prepare(mgicp_ctx* ctx, bool need_cov) {
  if (ctx->src.n == 0 || ctx->tgt.n == 0)
    return fail(ctx, MGICP_E_INVALID, "source and target clouds must be set before align");
  const int k = ctx->prm.k;
  if (static_cast<size_t>(k) > ctx->src.n || static_cast<size_t>(k) > ctx->tgt.n)
    return fail(ctx, MGICP_E_TOO_FEW_POINTS,
                "a cloud has fewer points than k_correspondences (PCL computeCovariances)");
  int rc;
  if (ctx->tgt.dirty && (rc = build_grid(ctx, ctx->tgt))) return rc;
  if (ctx->src.dirty && (rc = build_grid(ctx, ctx->src))) return rc;
  if (!need_cov) return MGICP_OK;
  // set_target's covariances still running count as current: the first sweep runs beside them and
  // joins them before its compaction (r05: the 1-NN search needs no covariance)
  if (!ctx->tgt.have_cov && !ctx->tgt_cov_pending && (rc = target_cov(ctx))) return rc;
  // set_source's covariances still running count as current: the sweep joins them (overlapped)
  const bool src_cur = ctx->src_cov_pending ||
                       (ctx->src.have_cov && ctx->src.cov_p0 == ctx->shard_p0() && ctx->src.cov_p1 == ctx->shard_p1());
  if (ctx->lazy_src_cov && !src_cur) {
    // computed per sweep for the points it accepts (cov_lazy); here only sized and marked empty
    if (!ctx->src_lazy_ready || ctx->src_lazy_p0 != ctx->shard_p0() || ctx->src_lazy_p1 != ctx->shard_p1()) {
      Cloud& c = ctx->src;
      const size_t ns = ctx->shard_p1() - ctx->shard_p0();
      HIPCK(c.cov.reserve(3 * c.n));
      c.cov_stride = c.n;
      HIPCK(ctx->cov_ok.reserve(std::max<size_t>(ns, 1)));
      HIPCK(ctx->cov_need.reserve(std::max<size_t>(ns, 1)));
      HIPCK(hipMemsetAsync(ctx->cov_ok.p, 0, std::max<size_t>(ns, 1), ctx->stream));
      ctx->src_lazy_ready = true;
      ctx->src_lazy_p0 = ctx->shard_p0();
      ctx->src_lazy_p1 = ctx->shard_p1();
    }
    return MGICP_OK;
  }
  if (!src_cur)
    if ((rc = compute_cov(ctx, ctx->src, ctx->shard_p0(), ctx->shard_p1()))) return rc;
  return MGICP_OK;
}

// guess-applied source cloud ("output" after transformPointCloud(output, output, guess))
int mgicp::set_output(mgicp_ctx* ctx, const Mat4& G) {
  float lo[3], hi[3];
  if (G.is_identity()) {
    ctx->d_out = ctx->src.pts.p;  // x*1 + y*0 + z*0 + 0 == x: identity leaves points intact
    for (int d = 0; d < 3; ++d) {
      lo[d] = ctx->src.lo[d];
      hi[d] = ctx->src.hi[d];
    }
  } else {
    HIPCK(ctx->src_out.reserve(ctx->src.n));
    HIPCK(launch_xform_points(ctx->src.pts.p, ctx->src.n, G.xf(), ctx->src_out.p, ctx->stream));
    ctx->d_out = ctx->src_out.p;
    // bbox of the transformed cloud (the Gauss-Newton expansion centre)
    if (int rc = bbox_to_host(ctx, ctx->src_out.p, ctx->src.n, lo, hi)) return rc;
  }
  for (int d = 0; d < 3; ++d) ctx->out_ctr[d] = static_cast<double>(0.5f * (lo[d] + hi[d]));
  ctx->last_guess = G;
  return MGICP_OK;
}

// One correspondence sweep (the loop body of computeTransformation before the BFGS call):
// exact 1-NN per source point, then a deterministic compaction of the accepted ones (exclusive
// scan of the flags, scatter in grid-sorted order) that computes their Mahalanobis matrices
// straight into the SoA streams.  `seed` uses the previous sweep's matches as 1-NN starting
// candidates (exact either way).
int mgicp::correspond(mgicp_ctx* ctx, const Mat4& T, const Mat4& G, bool seed) {
  const double thr = ctx->prm.max_corr_dist * ctx->prm.max_corr_dist;
  const size_t p0 = ctx->shard_p0(), p1 = ctx->shard_p1(), ns = p1 - p0;
  hipStream_t s = ctx->stream;
  const bool seeded = seed && ctx->seed_valid;
  HIPCK(hipMemsetAsync(ctx->flags.p + ns, 0, sizeof(uint32_t), s));
  const uint32_t* qp = query_perm(ctx);
  MGICP_TRACE_AT("corr: query order ready");
  if (ctx->vlist) {
    int rc = vl_prepare(ctx);
    if (rc) return rc;
  }
  MGICP_TRACE_AT("corr: lists prepared");
  // the compaction fused into a listed sweep: both clouds' covariances must be complete (or, lazy
  // source mode, marked per point) -- not on the first align after set_*, which runs the r03 sweep
  const bool fused = ctx->fuse_compact && sweep_listed(ctx) && ctx->tgt.have_cov &&
                     !ctx->tgt_cov_pending && !ctx->src_cov_pending &&
                     (ctx->src.have_cov || (ctx->lazy_src_cov && ctx->src_lazy_ready));
  FusedCompact fc{};
  if (fused) {
    HIPCK(ctx->vl_defer.reserve(std::max(chunk_count(ns), 1)));
    fc.cov_s = ctx->src.cov3();
    fc.cov_t = ctx->tgt.cov3();
    fc.R = rot_of(T, G);
    fc.cov_ok = ctx->src.have_cov ? nullptr : ctx->cov_ok.p;
    fc.ccnt = ctx->ccnt.p;
    fc.defer = ctx->vl_defer.p;
    fc.out = corr_soa(ctx);
  }
  // r08: a fused listed sweep queues its queries alone and hands ctr[1..3] to the host.  All zero: no cell
  // was requested, no query is pending and no chunk was deferred (a chunk is deferred exactly when it
  // holds a pending query or an accepted point without a covariance), so the streams are complete and
  // everything from vl_centre_kernel to the deferred compaction would find nothing to do.  Otherwise,
  // and for every other sweep, the sequence is the one before r08.  The decision is this rank's alone.
  const bool fast = fused && ctx->round_fast && ctx->h_round && ns > 0;
  bool clean = false;
  unsigned int c3[3] = {0, 0, 0};
  {
    ProfScope ps(ctx, kFamCorr);
    if (fast) {
      if (++ctx->round_stamp == 0) ctx->round_stamp = 1;
      const bool zero_ctr = ctx->vl_ctr_zero != ctx->vl_ctr.p;
      ctx->vl_ctr_zero = nullptr;
      HIPCK(launch_vl_queries(ctx->vl, ctx->d_out, p0, p1, T.xf(), thr, ctx->prev_pos.p, ctx->flags.p, s, &fc, zero_ctr,
                              ctx->d_round, ctx->round_stamp));
      if (int rc = wait_round(ctx, ctx->round_stamp, c3)) return rc;
      clean = !(c3[0] | c3[1] | c3[2]);
      if (clean)
        ctx->vl_ctr_zero = ctx->vl_ctr.p;  // ctr[4] is written by the builds only: still zero from the last fill
      else
        HIPCK(launch_vl_follow(ctx->tgt.view, ctx->vl, ctx->d_out, p0, p1, T.xf(), thr, seeded ? 1 : 0, ctx->prev_pos.p,
                               ctx->flags.p, ctx->cus, s));
    } else {
      HIPCK(launch_sweep(ctx, T, thr, seeded, qp, fused ? &fc : nullptr));
    }
  }
  ctx->seed_valid = true;
  MGICP_TRACE_AT("corr: sweep queued");
  if (int rc = report_sweep(ctx)) return rc;
  ctx->round_st[clean ? 0 : 1]++;
  if (c3[2]) ctx->round_st[2]++;
  if (c3[1]) ctx->round_st[3]++;
  if (clean) {
    ctx->have_corr = true;
    return MGICP_OK;
  }
  {
    int rc = cov_join_all(ctx);  // set_target's / set_source's covariances (they ran beside this sweep)
    if (rc) return rc;
    rc = cov_lazy(ctx);  // covariances of newly accepted source points (lazy source mode)
    MGICP_TRACE_AT("corr: lazy covariances queued (sweep drained)");
    if (rc) return rc;
  }
  {
    ProfScope ps(ctx, kFamCompact);
    // fused: only the chunks the sweep deferred (pending queries, lazy covariances computed above)
    HIPCK(launch_compact(ctx->d_out, ctx->tgt.view.pts, ctx->src.cov3(), ctx->tgt.cov3(), rot_of(T, G),
                         ctx->prev_pos.p, ctx->flags.p, p0, p1, ctx->ccnt.p, corr_soa(ctx), s,
                         fused ? ctx->vl_defer.p : nullptr, fused ? ctx->vl_ctr.p + 3 : nullptr, ctx->cus));
  }
  // no host round trip here: the correspondence count arrives with the first objective pass (its
  // count lane) and every consumer of the streams runs on the same stream
  ctx->have_corr = true;
  return MGICP_OK;
}

// Gauss-Newton mode, one device pass per outer iteration: the 74 moments of the objective over
// the accepted correspondences of the last sweep at T (Mahalanobis computed on the fly), finished
// over the fixed reduction tree (chunks, supers, all-gathered supers, fixed-order total), copied to
// the host.
int mgicp::moments_pass(mgicp_ctx* ctx, const Mat4& T, const Mat4& G, bool supers_only) {
  const size_t p0 = ctx->shard_p0(), p1 = ctx->shard_p1();
  hipStream_t s = ctx->stream;
  const int nch = chunk_count(p1 - p0);
  HIPCK(ctx->mpartial.reserve(std::max(nch, 1) * static_cast<size_t>(kMomVals)));
  HIPCK(ctx->msuper.reserve(std::max<long long>(ctx->max_supers(), 1) * static_cast<size_t>(kMomVals)));
  HIPCK(ctx->mred.reserve(kMomVals));
  {
    ProfScope ps(ctx, kFamMoments);
    if (nch > 0) {
      HIPCK(launch_gn_moments(ctx->d_out, ctx->tgt.view.pts, ctx->src.cov3(), ctx->tgt.cov3(),
                              rot_of(T, G), T.xf(), ctx->out_ctr, ctx->prev_pos.p, ctx->flags.p, p0,
                              p1, ctx->mpartial.p, chunk_grid_blocks(p1 - p0), s));
      HIPCK(launch_super_reduce(ctx->mpartial.p, nch, kMomVals, ctx->msuper.p, s));
    }
  }
  if (supers_only) return sync(ctx);
  int rc = combine_to_host(ctx, kMomVals, ctx->msuper.p, ctx->mom);
  if (rc) return rc;
  ctx->n_evals++;
  return MGICP_OK;
}

// getFitnessScore's chunk and super partials of this shard ([0] sum d2, [13] count) in spart
int mgicp::fitness_supers(mgicp_ctx* ctx, const Mat4& T, double max_range) {
  const size_t p0 = ctx->shard_p0(), p1 = ctx->shard_p1();
  const int nch = chunk_count(p1 - p0);
  if (nch == 0) return MGICP_OK;
  HIPCK(launch_fitness(ctx->tgt.view, ctx->src.pts.p, p0, p1, T.xf(), max_range, ctx->partial.p,
                       chunk_grid_blocks(p1 - p0), ctx->stream));
  HIPCK(launch_super_reduce(ctx->partial.p, nch, kRedVals, ctx->spart.p, ctx->stream));
  return MGICP_OK;
}

// =====================================================================================
// C-ABI
// =====================================================================================
extern "C" {

void mgicp_default_params(mgicp_params* p) {
  if (!p) return;
  p->max_iter = 100;        // GICPAlignment.cpp:30
  p->tf_eps = 4e-3;         // GICPAlignment.cpp:29
  p->rot_eps = 2e-3;        // PCL GICP rotation_epsilon_
  p->max_corr_dist = 4e-2;  // GICPAlignment.cpp:31
  p->gicp_eps = 1e-3;       // PCL GICP gicp_epsilon_
  p->k = 20;                // PCL GICP k_correspondences_
  p->max_inner_iter = 20;   // PCL GICP max_inner_iterations_
  p->solver = MGICP_SOLVER_PCL_BFGS;
  p->device = -1;
  p->fixed_iterations = 0;
}

int mgicp_device_count(int* n) {
  if (!n) return MGICP_E_INVALID;
  return hipGetDeviceCount(n) == hipSuccess ? MGICP_OK : MGICP_E_HIP;
}

int mgicp_create(mgicp_ctx** out, const mgicp_params* p) {
  if (!out) return MGICP_E_INVALID;
  *out = nullptr;
  std::unique_ptr<Graveyard> grave(new Graveyard());
  t_new_ctx_grave = grave.get();
  mgicp_ctx* ctx = new mgicp_ctx();
  t_new_ctx_grave = nullptr;
  ctx->grave = std::move(grave);
  // runtime environment (INTEGRATION.md "Environment"): deadlines of the pass transport and the fault
  // injection of the multi-rank tests only -- every alternative code path is a compile-time option
  // (Makefile `variant`) or a test's explicit mgicp_debug_option call, never an environment variable
  if (const char* sp = std::getenv("MGICP_SRV_STALL_PASS")) ctx->stall_pass = std::atoi(sp);
  if (const char* qp = std::getenv("MGICP_DEBUG_QUIT_PASS")) ctx->quit_pass = std::atoi(qp);
  if (const char* dl = std::getenv("MGICP_ROW_DEADLINE_MS")) {
    const double v = std::atof(dl);
    if (v > 0) ctx->row_deadline_ms = v;
  }
  if (const char* rd = std::getenv("MGICP_REMOTE_DEADLINE_S")) {
    const double v = std::atof(rd);
    if (v > 0) ctx->remote_deadline_s = v;
  }
  {
    const unsigned hc = std::thread::hardware_concurrency();
    ctx->host_threads = static_cast<int>(std::max(1u, std::min(8u, hc ? hc : 1u)));
  }
  if (p) ctx->prm = *p;
  else mgicp_default_params(&ctx->prm);
  int rc = check_params(ctx, ctx->prm);
  if (rc) {
    delete ctx;
    return rc;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    delete ctx;
    return MGICP_E_HIP;
  }
  if (ctx->prm.device >= 0) {
    if (ctx->prm.device >= ndev || hipSetDevice(ctx->prm.device) != hipSuccess) {
      delete ctx;
      return MGICP_E_INVALID;
    }
    ctx->device = ctx->prm.device;
  } else if (hipGetDevice(&ctx->device) != hipSuccess) {
    delete ctx;
    return MGICP_E_HIP;
  }
  if (hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess)
    ctx->cus = 0;  // no resident server
  ctx->tgt.want_empty_map = true;  // correspondence / fitness queries start off the surface
  ctx->tgt.want_seed_map = true;  // first 1-NN sweep seeded from a nearest non-empty cell
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return MGICP_E_HIP;
  }
  MGICP_TRACE_AT("create: stream");
  bool ok = hipHostMalloc(reinterpret_cast<void**>(&ctx->h_small), kSmallBytes,
                          hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
            hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_small), ctx->h_small, 0) == hipSuccess;
  MGICP_TRACE_AT("create: pinned words");
  ok = ok && preload_kernels(ctx->h_small, kSmallBytes, ctx->stream) == hipSuccess;
  MGICP_TRACE_AT("create: kernels loaded");
  ok = ok && HostUploader::instance().init(ctx->host_threads) == hipSuccess;
  MGICP_TRACE_AT("create: upload staging");
  if (!ok) {
    if (ctx->h_small) (void)hipHostFree(ctx->h_small);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MGICP_E_HIP;
  }
  // the pass path's pinned command / result words and the BAR command block (its memset is
  // synchronous): here, not in the first align, where they waited for the covariance head start
  (void)ensure_host_red(ctx);  // (retried by the first align if it failed)
  MGICP_TRACE_AT("create: pass words + BAR block");
  // the stream of the covariance head start (created here: a stream's creation costs milliseconds
  // of host time, which set_* would otherwise pay before the launch).  A CU mask on it (leaving CUs to
  // the main stream) was measured -0.5 to -1.4 ms on new clouds (profiles/r04/ncab1) but a CU mask
  // belongs to the hardware queue, which past GPU_MAX_HW_QUEUES streams share: not used.
  hipError_t se = hipSuccess;
  if (ctx->async_tgt) se = hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking);
  if (ctx->async_tgt && (se != hipSuccess ||
                         hipEventCreateWithFlags(&ctx->aux_ev[0], hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&ctx->aux_ev[1], hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&ctx->aux_ev[2], hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&ctx->aux_ev[3], hipEventDisableTiming) != hipSuccess)) {
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    for (hipEvent_t& ev : ctx->aux_ev)
      if (ev) (void)hipEventDestroy(ev), ev = nullptr;
    ctx->aux_stream = nullptr;
  }
  MGICP_TRACE_AT("create: aux stream");
  *out = ctx;
  return MGICP_OK;
}

int mgicp_set_params(mgicp_ctx* ctx, const mgicp_params* p) {
  if (!ctx || !p) return MGICP_E_INVALID;
  int rc = check_params(ctx, *p);
  if (rc) return rc;
  if ((rc = cov_join_all(ctx))) return rc;  // a pending covariance launch uses the old k / eps
  const bool cov_change = p->k != ctx->prm.k || p->gicp_eps != ctx->prm.gicp_eps;
  const int dev = ctx->device;
  ctx->prm = *p;
  ctx->prm.device = dev;
  if (cov_change) {
    ctx->src.have_cov = false;
    ctx->tgt.have_cov = false;
    ctx->src_lazy_ready = false;
  }
  return MGICP_OK;
}

const char* mgicp_last_error(const mgicp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void mgicp_destroy(mgicp_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  cancel_gated(ctx);
  if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
  // a head-start launch chain that ran to its end on the aux stream completed the target's covariances
  const bool tgt_cov_done = ctx->tgt.have_cov || (ctx->tgt_cov_pending && !ctx->tgt.dirty);
  ctx->tgt_cov_pending = ctx->src_cov_pending = false;
  (void)hipStreamSynchronize(ctx->stream);
  srv_release(ctx);
  tcache_donate(ctx, tgt_cov_done);  // r05: the target's grid, covariances and lists outlive the context
  ctx->f_flags.release(); ctx->f_pos.release(); ctx->f_rgba_in.release(); ctx->f_rgba.release();
  ctx->f_rgba2.release(); ctx->f_vox.release(); ctx->f_vox2.release(); ctx->f_keep.release();
  ctx->f_count.release();
  ctx->cc_parent.release(); ctx->cc_root.release(); ctx->cc_min.release(); ctx->cc_members.release();
  ctx->cc_tests.release();
  for (Cloud* c : {&ctx->src, &ctx->tgt, &ctx->aux, &ctx->qry}) {
    c->raw.release(); c->orig.release(); c->pts.release(); c->perm.release();
    c->cell_start.release(); c->cov.release(); c->empty_dist.release(); c->pairs.release();
    c->seed.release(); c->seed_scratch.release();
  }
  ctx->src_out.release();
  ctx->qperm.release();
  ctx->aq_keys.release(); ctx->aq_keys_sorted.release(); ctx->aq_vals.release(); ctx->aq_scratch.release();
  ctx->partial.release(); ctx->red.release(); ctx->mpartial.release(); ctx->mred.release(); ctx->counts.release(); ctx->keys.release();
  ctx->keys_sorted.release(); ctx->vals.release(); ctx->scratch.release(); ctx->u64.release();
  ctx->fpartial.release();
  ctx->knn_fb.release();
  ctx->tickets.release();
  ctx->tickets_n = 0;
  ctx->ccnt.release(); ctx->spart.release(); ctx->gath.release(); ctx->msuper.release();
  ctx->prev_pos.release(); ctx->flags.release();
  ctx->vl_cell.release(); ctx->vl_pool.release(); ctx->vl_ctr.release();
  ctx->vl_build.release(); ctx->vl_bcentre.release(); ctx->vl_pend.release(); ctx->vl_defer.release();
  ctx->cov_ok.release(); ctx->cov_need.release();
  ctx->aux_cnt.release(); ctx->knn_fb2.release();
  ctx->tpart.release();
  ctx->tpart_n = 0;
  ctx->corr_f.release(); ctx->corr_d.release();
  ctx->xyz_dev.release();
  if (ctx->mail) (void)hipFree(ctx->mail);
  if (ctx->h_red) (void)hipHostFree(ctx->h_red);
  if (ctx->h_cmd) (void)hipHostFree(ctx->h_cmd);
  if (ctx->h_round) (void)hipHostFree(ctx->h_round);
  if (ctx->h_gtrace) (void)hipHostFree(ctx->h_gtrace);
  if (ctx->h_ptimes) (void)hipHostFree(ctx->h_ptimes);
  if (ctx->h_rows) (void)hipHostFree(ctx->h_rows);
  xgmi_detach(ctx);
  if (ctx->xstream && ctx->xstream_own) (void)hipStreamDestroy(ctx->xstream);
  if (ctx->h_xtot) (void)hipHostFree(ctx->h_xtot);
  if (ctx->have_shm) {
    (void)hipHostUnregister(ctx->shm.base);
    shm::detach(ctx->shm);
    ctx->have_shm = false;
  }
  if (ctx->bar_cmd) (void)hipFree(ctx->bar_cmd);
  if (ctx->h_small) (void)hipHostFree(ctx->h_small);
  prof_resolve(ctx);
  srv_resolve(ctx);
  for (hipEvent_t e : ctx->pool) (void)hipEventDestroy(e);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
  ctx->grave->flush();
  for (hipEvent_t e : ctx->aux_ev)
    if (e) (void)hipEventDestroy(e);
  delete ctx;
}

int mgicp_set_target(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride) {
  return set_cloud(ctx, true, xyz, n, stride, false);
}
int mgicp_set_source(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride) {
  return set_cloud(ctx, false, xyz, n, stride, false);
}
int mgicp_set_target_device(mgicp_ctx* ctx, const float* d_xyz, size_t n, size_t stride) {
  return set_cloud(ctx, true, d_xyz, n, stride, true);
}
int mgicp_set_source_device(mgicp_ctx* ctx, const float* d_xyz, size_t n, size_t stride) {
  return set_cloud(ctx, false, d_xyz, n, stride, true);
}

int mgicp_align(mgicp_ctx* ctx, const float guess_cm[16], float out_T_cm[16], mgicp_result* res) {
  if (!ctx || !out_T_cm) return MGICP_E_INVALID;
  if (ctx->nranks > 1 && !ctx->comm && !ctx->have_shm)
    return fail(ctx, MGICP_E_INVALID, "detached shard context: only the debug entry points are available");
  HIPCK(hipSetDevice(ctx->device));
  mgicp_result r;
  std::memset(&r, 0, sizeof(r));
  const double t0 = now_ms();
  MGICP_TRACE_AT("align: begin");
  AlignDrain drain{ctx};
  int rc = prepare(ctx, true);
  if (rc) return rc;
  MGICP_TRACE_AT("align: prepared");
  rc = ensure_iter_buffers(ctx);
  if (rc) return rc;
  MGICP_TRACE_AT("align: iteration buffers ready");
  const double t1 = now_ms();
  const Mat4 G = guess_cm ? Mat4::from_cm(guess_cm) : Mat4::identity();
  if ((rc = set_output(ctx, G))) return rc;

  Mat4 T = Mat4::identity(), prev = Mat4::identity();
  ctx->trace.clear();
  ctx->n_evals = 0;
  ctx->srv_degraded = false;  // a take-over degrades the rest of one align only
  int nr_iterations = 0;
  bool converged = false;
  int solver_rc = MGICP_OK;
  while (!converged) {
    const bool gn_mode = ctx->prm.solver == MGICP_SOLVER_GN;
    rc = gn_mode ? correspond_gn(ctx, T, G, nr_iterations > 0)
                 : correspond(ctx, T, G, nr_iterations > 0);
    if (rc) return rc;
    prev = T;
    int ncorr = 0;
    MGICP_TRACE_AT("align: sweep done");
    rc = gn_mode ? estimate_gn(ctx, T, &ncorr) : estimate_bfgs(ctx, T, &ncorr);
    MGICP_TRACE_AT("align: solve done");
    r.n_corr = ncorr;
    if (rc == MGICP_E_SOLVER) {  // PCLException caught: converged_ stays false
      T = prev;
      solver_rc = rc;
      break;
    }
    if (rc) return rc;
    double delta = 0.;
    for (int k = 0; k < 4; ++k)
      for (int l = 0; l < 4; ++l) {
        const double ratio = (k < 3 && l < 3) ? 1. / ctx->prm.rot_eps : 1. / ctx->prm.tf_eps;
        const double c_delta = ratio * static_cast<double>(std::fabs(prev.m[k][l] - T.m[k][l]));
        if (c_delta > delta) delta = c_delta;
      }
    float tcm[16];
    T.to_cm(tcm);
    ctx->trace.insert(ctx->trace.end(), tcm, tcm + 16);
    nr_iterations++;
    const bool stop = ctx->prm.fixed_iterations
                          ? nr_iterations >= ctx->prm.max_iter
                          : (nr_iterations >= ctx->prm.max_iter || delta < 1);
    if (stop) {
      converged = true;
      prev = T;
    }
  }
  // polled passes leave their kernels' completion unobserved: drain the stream once
  if ((rc = sync(ctx))) return rc;
  drain.armed = false;
  if (!ctx->tgt_cov_pending && !ctx->src_cov_pending) ctx->grave->flush();  // a quiet point
  if (ctx->vl_valid) ctx->vl_groups++;
  report_pass_times(ctx);
  // final_transformation_ = previous_transformation_ (3x3) * guess (3x3); t = prev t + guess t
  Mat4 F = Mat4::identity();
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      float a = prev.m[i][0] * G.m[0][j];
      a = a + prev.m[i][1] * G.m[1][j];
      a = a + prev.m[i][2] * G.m[2][j];
      F.m[i][j] = a;
    }
  for (int i = 0; i < 3; ++i) F.m[i][3] = prev.m[i][3] + G.m[i][3];
  F.to_cm(out_T_cm);
  const double t2 = now_ms();
  r.converged = converged ? 1 : 0;
  r.iterations = nr_iterations;
  r.n_evals = ctx->n_evals;
  r.ms_upload = ctx->ms_upload_pending;
  ctx->ms_upload_pending = 0;
  r.ms_prep = t1 - t0;
  r.ms_loop = t2 - t1;
  r.ms_total = t2 - t0 + r.ms_upload;
  if (res) *res = r;
  if (solver_rc) return fail(ctx, solver_rc, "GICP solver threw (fewer than 4 correspondences or BFGS failure)");
  return MGICP_OK;
}

int mgicp_fitness(mgicp_ctx* ctx, const float T_cm[16], double max_range, double* out) {
  if (!ctx || !T_cm || !out) return MGICP_E_INVALID;
  if (ctx->nranks > 1 && !ctx->comm && !ctx->have_shm)
    return fail(ctx, MGICP_E_INVALID, "detached shard context: only the debug entry points are available");
  HIPCK(hipSetDevice(ctx->device));
  int rc = prepare(ctx, false);
  if (rc) return rc;
  if ((rc = ensure_iter_buffers(ctx))) return rc;
  if (!(max_range > 0)) max_range = 1.7976931348623157e308;
  const Mat4 T = Mat4::from_cm(T_cm);
  if ((rc = fitness_supers(ctx, T, max_range))) return rc;
  double tot[kRedVals];
  if ((rc = combine_to_host(ctx, kRedVals, ctx->spart.p, tot))) return rc;
  const double nr = tot[13];
  *out = nr > 0 ? tot[0] / nr : 1.7976931348623157e308;
  return MGICP_OK;
}

}  // extern "C"
