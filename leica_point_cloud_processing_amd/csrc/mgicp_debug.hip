// mgicp_debug.hip -- the test, benchmark and diagnostic entry points of libmgicp.so
// (include/mi355x_gicp_debug.h): introspection for the parity tests, pass timing and counters for
// bench.py, and the per-context switches between the engine's forms.  Not part of the drop-in: the
// product calls of include/mi355x_gicp.h live in mgicp_engine.hip and the host files beside it
// (mgicp_clouds.hip, mgicp_pass.hip, mgicp_fod.hip, mgicp_features.hip, mgicp_comm.hip), whose helpers these reach through
// mgicp_ctx.hpp.
#pragma clang fp contract(off)

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mi355x_gicp_debug.h"
#include "mgicp_ctx.hpp"

extern "C" {

int mgicp_debug_pass_stats(mgicp_ctx* ctx, long long out[9]) {
  if (!ctx || !out) return MGICP_E_INVALID;
  for (int i = 0; i < kStCount; ++i) out[i] = ctx->st[i];
  return MGICP_OK;
}

int mgicp_debug_round_stats(mgicp_ctx* ctx, long long out[4]) {
  if (!ctx || !out) return MGICP_E_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = ctx->round_st[i];
  return MGICP_OK;
}

int mgicp_debug_server_time(mgicp_ctx* ctx, double* out_ms, long long* out_passes, long long* out_launches,
                            int reset) {
  if (!ctx || !out_ms || !out_passes || !out_launches) return MGICP_E_INVALID;
  *out_ms = ctx->srv_time_ms;
  *out_passes = ctx->srv_time_passes;
  *out_launches = ctx->srv_time_launches;
  if (reset) {
    ctx->srv_time_ms = 0;
    ctx->srv_time_passes = ctx->srv_time_launches = 0;
  }
  return MGICP_OK;
}

int mgicp_debug_target_cov_slice(mgicp_ctx* ctx, int nranks, int rank, double* out_c6) {
  if (!ctx || !out_c6 || nranks < 1 || rank < 0 || rank >= nranks) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = prepare(ctx, false);
  if (rc || (rc = cov_join_all(ctx))) return rc;  // set_target's k-NN launch still writes tgt.cov
  Cloud& t = ctx->tgt;
  const size_t N = static_cast<size_t>(nranks), r = static_cast<size_t>(rank);
  const size_t cnt = (t.n + N - 1) / N;
  const size_t a = std::min(t.n, r * cnt), b = std::min(t.n, (r + 1) * cnt);
  // target_cov's slice call, verbatim: the same range, the same N * cnt array layout
  if ((rc = compute_cov(ctx, t, a, b, N * cnt))) return rc;
  t.have_cov = false;  // only a slice is current: the next align recomputes the target's covariances
  const size_t m = b - a;
  std::vector<double2> h(3 * std::max<size_t>(m, 1));
  if (m) {
    const Cov3 c = t.cov3();
    HIPCK(hipMemcpyAsync(h.data(), c.a + a, m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    HIPCK(hipMemcpyAsync(h.data() + m, c.b + a, m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    HIPCK(hipMemcpyAsync(h.data() + 2 * m, c.c + a, m * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
  }
  if ((rc = sync(ctx))) return rc;
  for (size_t i = 0; i < m; ++i) {  // grid-sorted order, as the arrays hold them
    double* o = out_c6 + 6 * i;
    o[0] = h[i].x; o[1] = h[i].y; o[2] = h[m + i].x; o[3] = h[m + i].y; o[4] = h[2 * m + i].x; o[5] = h[2 * m + i].y;
  }
  return static_cast<int>(m);
}

int mgicp_debug_vlist_stats(mgicp_ctx* ctx, long long out[8]) {
  if (!ctx || !out) return MGICP_E_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (!ctx->vlist || !ctx->vl_valid || ctx->vl_off || !ctx->vl_alloc) return MGICP_OK;
  HIPCK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  unsigned int c3[3];
  HIPCK(hipMemcpyAsync(c3, ctx->vl_ctr.p, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  HIPCK(ctx->u64.reserve(64));
  HIPCK(launch_vl_stats(ctx->vl, ctx->vl_ncells, ctx->u64.p, s));
  unsigned long long st[64];
  HIPCK(hipMemcpyAsync(st, ctx->u64.p, sizeof(st), hipMemcpyDeviceToHost, s));
  int rc = sync(ctx);
  if (rc) return rc;
  out[0] = c3[1];
  out[1] = c3[2];
  out[2] = static_cast<long long>(st[0]);
  out[3] = static_cast<long long>(st[1]);
  out[4] = static_cast<long long>(st[2]);
  out[5] = static_cast<long long>(st[3]);
  out[6] = c3[0];
  out[7] = static_cast<long long>(ctx->vl_ncells);
  return MGICP_OK;
}

// The fine grid's layout, the list counters and (state / length / offset non-null) every fine cell's
// state class, true list length and pool offset: host work over device-to-host copies of the state
// words, the counters and the long lists' header entries (4 bytes each); no kernel.
int mgicp_debug_vlist_layout(mgicp_ctx* ctx, double out[24], uint8_t* state, uint32_t* length, uint32_t* offset,
                             size_t cap) {
  if (!ctx || !out) return MGICP_E_INVALID;
  for (int i = 0; i < 24; ++i) out[i] = 0.0;
  out[8] = ctx->prm.max_corr_dist;
  out[9] = ctx->tgt.view.h;
  if (!ctx->vlist || !ctx->vl_valid) return MGICP_OK;
  const VListView& v = ctx->vl;
  out[8] = v.gate;
  out[10] = ctx->vl_off ? 1.0 : 0.0;
  if (ctx->vl_off) return MGICP_OK;
  out[0] = v.ox; out[1] = v.oy; out[2] = v.oz;
  out[3] = v.c;
  out[4] = v.es;
  out[5] = v.nx; out[6] = v.ny; out[7] = v.nz;
  out[17] = static_cast<double>(ctx->vl_ncells);
  out[19] = v.inv_c;
  if (!ctx->vl_alloc) return MGICP_OK;
  out[18] = 1.0;
  HIPCK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  unsigned int c8[8];
  HIPCK(hipMemcpyAsync(c8, ctx->vl_ctr.p, sizeof(c8), hipMemcpyDeviceToHost, s));
  int rc = sync(ctx);
  if (rc) return rc;
  out[11] = v.pool_cap;
  out[12] = c8[0];
  out[13] = v.build_cap;
  out[14] = c8[1];
  out[15] = c8[2];
  out[16] = c8[4];
  if (!state && !length && !offset) return MGICP_OK;
  const size_t nc = ctx->vl_ncells;
  if (cap < nc) return fail(ctx, MGICP_E_INVALID, "debug_vlist_layout: cap below the fine grid's cell count");
  std::vector<uint32_t> cell(nc);
  HIPCK(hipMemcpyAsync(cell.data(), ctx->vl_cell.p, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if ((rc = sync(ctx))) return rc;
  std::vector<size_t> lng;  // the long lists' cells: their true counts are in the pool (header entry, x bits)
  for (size_t i = 0; i < nc; ++i) {
    const uint32_t c = cell[i];
    uint8_t st = 5;
    uint32_t len = 0, off = 0;
    if (c == kVlNotBuilt) st = 0;
    else if (c == kVlRequested) st = 2;
    else if (c == kVlOverflow) st = 4;
    else if (c == kVlReject) st = 3;
    else if (c >= kVlTouched) st = 1;
    else {
      off = (c >> 6) << 2;
      len = c & 63u;
      if (len == static_cast<uint32_t>(kVlLong)) {
        if (off >= v.pool_cap) return fail(ctx, MGICP_E_HIP, "debug_vlist_layout: a long list starts past the pool");
        if (length) lng.push_back(i);
      }
    }
    if (state) state[i] = st;
    if (length) length[i] = len;
    if (offset) offset[i] = off;
  }
  // one 4-byte copy per long list (its header's count), not the pool
  for (size_t i : lng)
    HIPCK(hipMemcpyAsync(&length[i], &ctx->vl_pool.p[(cell[i] >> 6) << 2].x, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (!lng.empty() && (rc = sync(ctx))) return rc;
  return MGICP_OK;
}

// r06: the objective's stream order -- original indices of this rank's source points in the order the
// compacted streams (and so every sum's fixed tree) visit them; the oracle's summation-order ledger runs
// the engine's tree over it (oracle/gicp_ref.c ref_set_sum_order).  Returns the count (<= cap written).
int mgicp_debug_source_order(mgicp_ctx* ctx, uint32_t* out, size_t cap) {
  if (!ctx || !out) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = prepare(ctx, false);
  if (rc) return rc;
  const size_t p0 = ctx->shard_p0(), ns = ctx->shard_p1() - p0;
  if (cap < ns) return fail(ctx, MGICP_E_INVALID, "debug_source_order: cap below the shard's point count");
  HIPCK(hipMemcpyAsync(out, ctx->src.perm.p + p0, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = sync(ctx))) return rc;
  return static_cast<int>(ns);
}

int mgicp_debug_covariances(mgicp_ctx* ctx, int which, double* out_c6) {
  if (!ctx || !out_c6 || (which != 0 && which != 1)) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = prepare(ctx, true);
  if (rc) return rc;
  // both clouds: prepare counts set_target's running covariances as current
  if ((rc = cov_join_all(ctx))) return rc;
  if (which == 0 &&!(ctx->src.have_cov && ctx->src.cov_p0 == ctx->shard_p0() && ctx->src.cov_p1 == ctx->shard_p1())) {
    // every source covariance (lazy mode computes only the accepted points' ones)
    if ((rc = compute_cov(ctx, ctx->src, ctx->shard_p0(), ctx->shard_p1()))) return rc;
    if (ctx->src_lazy_ready) HIPCK(hipMemsetAsync(ctx->cov_ok.p, 1, ctx->shard_p1() - ctx->shard_p0(), ctx->stream));
  }
  Cloud& cl = which ? ctx->tgt : ctx->src;
  const size_t n = cl.n;
  const size_t st = cl.cov_stride;
  std::vector<double2> h(3 * st);
  std::vector<uint32_t> perm(n);
  HIPCK(hipMemcpyAsync(h.data(), cl.cov.p, 3 * st * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
  HIPCK(hipMemcpyAsync(perm.data(), cl.perm.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = sync(ctx))) return rc;
  for (size_t p = 0; p < n; ++p) {
    double* o = out_c6 + 6 * static_cast<size_t>(perm[p]);
    o[0] = h[p].x; o[1] = h[p].y;
    o[2] = h[st + p].x; o[3] = h[st + p].y;
    o[4] = h[2 * st + p].x; o[5] = h[2 * st + p].y;
  }
  return MGICP_OK;
}

static int debug_corr(mgicp_ctx* ctx, const float T_cm[16], bool seeded, int* out_tgt, double* out_M6) {
  if (!ctx || !T_cm) return MGICP_E_INVALID;
  if (seeded && !ctx->seed_valid) return fail(ctx, MGICP_E_INVALID, "no previous sweep to seed from");
  HIPCK(hipSetDevice(ctx->device));
  int rc = prepare(ctx, true);
  if (rc) return rc;
  if ((rc = ensure_iter_buffers(ctx))) return rc;
  const size_t n = ctx->src.n;
  const Mat4 G = Mat4::identity();
  if ((rc = set_output(ctx, G))) return rc;
  if ((rc = correspond(ctx, Mat4::from_cm(T_cm), G, seeded))) return rc;
  if (ctx->vl_valid) ctx->vl_groups++;
  const size_t p0 = ctx->shard_p0(), p1 = ctx->shard_p1(), ns = p1 - p0;
  std::vector<uint32_t> nn(ns), flag(ns), perm(n), tperm(ctx->tgt.n);
  std::vector<uint32_t> ccnt(static_cast<size_t>(chunk_count(ns)));
  HIPCK(hipMemcpyAsync(nn.data(), ctx->prev_pos.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCK(hipMemcpyAsync(flag.data(), ctx->flags.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (!ccnt.empty())
    HIPCK(hipMemcpyAsync(ccnt.data(), ctx->ccnt.p, ccnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCK(hipMemcpyAsync(perm.data(), ctx->src.perm.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCK(hipMemcpyAsync(tperm.data(), ctx->tgt.perm.p, ctx->tgt.n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  const size_t cap = ctx->corr_cap;
  std::vector<double> M(6 * cap);
  HIPCK(hipMemcpyAsync(M.data(), ctx->corr_d.p, 6 * cap * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = sync(ctx))) return rc;
  int cnt = 0;
  size_t rank = 0;  // accepted before k in k's chunk
  for (size_t p = p0; p < p1; ++p) {
    const size_t i = perm[p], k = p - p0;
    if (k % kChunkPts == 0) rank = 0;
    const bool ok = flag[k] != 0;
    if (out_tgt) out_tgt[i] = ok ? static_cast<int>(tperm[nn[k]]) : -1;
    if (out_M6) {
      double* o = out_M6 + 6 * i;
      const size_t at = (k / kChunkPts) * kChunkPts + rank;  // the chunk's run of the streams
      for (int v = 0; v < 6; ++v) o[v] = ok ? M[v * cap + at] : 0.0;
    }
    if (ok) {
      cnt++;
      rank++;
    }
  }
  for (size_t c = 0; c < ccnt.size(); ++c) {  // the compaction's counts agree with the flags
    size_t m = 0;
    for (size_t k = c * kChunkPts; k < std::min(ns, (c + 1) * kChunkPts); ++k) m += flag[k] != 0;
    if (m != ccnt[c]) return fail(ctx, MGICP_E_HIP, "chunk counts disagree with the sweep's flags");
  }
  return cnt;
}

int mgicp_debug_correspondences(mgicp_ctx* ctx, const float T_cm[16], int* out_tgt, double* out_M6) {
  return debug_corr(ctx, T_cm, false, out_tgt, out_M6);
}

int mgicp_debug_correspondences_seeded(mgicp_ctx* ctx, const float T_cm[16], int* out_tgt, double* out_M6) {
  return debug_corr(ctx, T_cm, true, out_tgt, out_M6);
}

int mgicp_debug_fdf(mgicp_ctx* ctx, const double x[6], double* f, double g6[6]) {
  if (!ctx || !x || !ctx->have_corr) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  Vec6 xv, gv;
  for (int i = 0; i < 6; ++i) xv[i] = x[i];
  double fv = 0;
  int rc = fdf_at(ctx, xv, fv, gv);
  if (rc) return rc;
  if (f) *f = fv;
  if (g6)
    for (int i = 0; i < 6; ++i) g6[i] = gv[i];
  return MGICP_OK;
}

int mgicp_debug_fdf_sums(mgicp_ctx* ctx, const double x[6], double out16[16]) {
  if (!ctx || !x || !out16 || !ctx->have_corr) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  Vec6 xv;
  for (int i = 0; i < 6; ++i) xv[i] = x[i];
  return fdf_sums_at(ctx, xv, out16);
}

int mgicp_debug_fdf_sums_run(mgicp_ctx* ctx, const double* xs, int n, double* out16n) {
  if (!ctx || !xs || !out16n || n < 1 || n > 4096 || !ctx->have_corr) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  std::vector<Vec6> xv(static_cast<size_t>(n));
  for (int k = 0; k < n; ++k)
    for (int i = 0; i < 6; ++i) xv[k][i] = xs[6 * k + i];
  return fdf_sums_run_at(ctx, xv.data(), n, out16n);
}

int mgicp_debug_pass_bench(mgicp_ctx* ctx, const double x[6], int npasses, int mode, double* out_ms,
                           double out16[16]) {
  if (!ctx || !x || npasses < 1 || npasses > 100000 || (mode != 0 && mode != 1) || !ctx->have_corr)
    return MGICP_E_INVALID;
  if (ctx->comm || ctx->nranks != 1 || ctx->have_shm)
    return fail(ctx, MGICP_E_INVALID, "pass bench: single-rank contexts only");
  HIPCK(hipSetDevice(ctx->device));
  int rc = sync(ctx);  // cancels any queued pass / live server
  if (rc) return rc;
  if ((rc = ensure_host_red(ctx))) return rc;
  Vec6 xv;
  for (int i = 0; i < 6; ++i) xv[i] = x[i];
  const Xf34 A = apply_state(xv).xf();
  const size_t ns = ctx->shard_p1() - ctx->shard_p0();
  const CorrSoA c = corr_soa(ctx);
  hipEvent_t a = nullptr, b = nullptr;
  HIPCK(hipEventCreate(&a));
  HIPCK(hipEventCreate(&b));
  HIPCK(hipEventRecord(a, ctx->stream));
  hipError_t e = hipSuccess;
  const bool rows = mode == 0 && ctx->host_rows;
  if (rows && (rc = ensure_rows(ctx))) return rc;
  if (rows) HIPCK(hipMemsetAsync(ctx->tickets.p, 0, ctx->tickets_n * sizeof(unsigned int), ctx->stream));
  if (mode == 0) {
    const int cap = ctx->srv_cus > 0 ? std::min(ctx->srv_cus, ctx->cus) : ctx->cus;
    const int nb = fdf_server_blocks(ns, cap);
    if (nb <= 0) {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
      return fail(ctx, MGICP_E_INVALID, "pass bench: shard not servable by the resident server");
    }
    const unsigned long long seq0 = ++ctx->pass_seq;
    const RowView rv = row_view(ctx);
    e = launch_fdf_server(c, ctx->ccnt.p, ns, ctx->partial.p, ctx->spart.p, ctx->tickets.p,
                          ctx->d_h_red, ctx->d_flag, seq0, ctx->d_cmd, ctx->mail, ctx->gate_timeout, ctx->d_ptimes,
                          npasses, A, rows ? rv.dev_rows(0) : nullptr, rv.stride, nb, 1, -1, ctx->tpart.p, ctx->stream);
    ctx->pass_seq = seq0 + static_cast<unsigned long long>(npasses);  // the closing cancel's stamp too
  } else {
    const int nb = fdf_grid_blocks(ns, kFdfMaxBlocks);
    for (int k = 0; k < npasses && e == hipSuccess; ++k)
      e = launch_fdf_soa(c, ctx->ccnt.p, ns, A, ctx->partial.p, ctx->spart.p, nb, ctx->tickets.p,
                         ctx->d_h_red, k & 1, ctx->d_flag, ++ctx->pass_seq, ctx->stream);
  }
  if (e == hipSuccess) e = hipEventRecord(b, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  HIPCK(e);
  if (MGICP_PASS_DIAG && mode == 0) {
    PassCmd m{};
    HIPCK(hipMemcpy(&m, ctx->mail, sizeof(PassCmd), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[srv-debug] seq0 %llu npasses %d ms %.3f | mail:", ctx->pass_seq - npasses, npasses, ms);
    for (int i = 0; i < 16; ++i)
      std::fprintf(stderr, " %x:%x", static_cast<unsigned>(m.h[i] >> 32), static_cast<unsigned>(m.h[i]));
    std::fprintf(stderr, "\n");
    if (ctx->h_ptimes)
      for (unsigned long long q = ctx->pass_seq - npasses; q < ctx->pass_seq + 1; ++q)
        std::fprintf(stderr, "[srv-debug] pass %llu: gate exit %llu finish %llu\n", q, ctx->h_ptimes[2 * (q & 1023)],
                     ctx->h_ptimes[2 * (q & 1023) + 1]);
  }
  if (rows) {
    // the host-row tickets are left as multiples of the supers' sizes: re-arm them
    HIPCK(hipMemsetAsync(ctx->tickets.p, 0, ctx->tickets_n * sizeof(unsigned int), ctx->stream));
    double tot[kRedVals];
    // the timing form stamps each pass's rows with its sequence number | 2^31
    const Xf34 unused{};
    if ((rc = wait_rows(ctx, static_cast<unsigned int>(ctx->pass_seq - 1) | 0x80000000u, unused, tot, false))) return rc;
    if ((rc = sync(ctx))) return rc;
    if (out16) std::memcpy(out16, tot, kRedVals * sizeof(double));
  } else {
    if (__atomic_load_n(ctx->h_flag, __ATOMIC_ACQUIRE) != ctx->pass_seq - (mode == 0 ? 1 : 0))
      return fail(ctx, MGICP_E_HIP, "pass bench: the last pass did not publish its sums");
    if (out16) std::memcpy(out16, ctx->h_red, kRedVals * sizeof(double));
  }
  if (out_ms) *out_ms = static_cast<double>(ms) / npasses;
  return MGICP_OK;
}

int mgicp_debug_moments(mgicp_ctx* ctx, const float T_cm[16], double out80[80]) {
  if (!ctx || !T_cm || !out80 || !ctx->seed_valid) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = moments_pass(ctx, Mat4::from_cm(T_cm), ctx->last_guess);
  if (rc) return rc;
  std::memcpy(out80, ctx->mom, kMomVals * sizeof(double));
  return MGICP_OK;
}

int mgicp_debug_supers(mgicp_ctx* ctx, int kind, const double* arg, double* out, int cap) {
  if (!ctx || !arg || !out || kind < 0 || kind > 2) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const long long nsup = ctx->nsup_local();
  if (nsup > cap) return fail(ctx, MGICP_E_INVALID, "debug_supers: output too small");
  const int nv = kind == 1 ? kMomVals : kRedVals;
  float Tcm[16];
  for (int i = 0; i < 16 && kind != 0; ++i) Tcm[i] = static_cast<float>(arg[i]);
  int rc;
  const double* sup = ctx->spart.p;
  if (kind == 0) {  // one objective pass at x over the last sweep, stopped at the supers
    if (!ctx->have_corr) return fail(ctx, MGICP_E_INVALID, "no correspondence sweep yet");
    cancel_gated(ctx);
    Vec6 x;
    for (int i = 0; i < 6; ++i) x[i] = arg[i];
    const size_t ns = ctx->shard_p1() - ctx->shard_p0();
    // host-row passes leave the tickets as multiples of their supers' sizes
    HIPCK(hipMemsetAsync(ctx->tickets.p, 0, ctx->tickets_n * sizeof(unsigned int), ctx->stream));
    HIPCK(launch_fdf_soa(corr_soa(ctx), ctx->ccnt.p, ns, apply_state(x).xf(), ctx->partial.p,
                         ctx->spart.p, fdf_grid_blocks(ns, kFdfMaxBlocks), ctx->tickets.p, nullptr, 0,
                         nullptr, 0, ctx->stream));
  } else if (kind == 1) {
    if (!ctx->seed_valid) return fail(ctx, MGICP_E_INVALID, "no correspondence sweep yet");
    if ((rc = moments_pass(ctx, Mat4::from_cm(Tcm), ctx->last_guess, true))) return rc;
    sup = ctx->msuper.p;
  } else {
    if ((rc = prepare(ctx, false)) || (rc = ensure_iter_buffers(ctx))) return rc;
    const double mr = arg[16] > 0 ? arg[16] : 1.7976931348623157e308;
    if ((rc = fitness_supers(ctx, Mat4::from_cm(Tcm), mr))) return rc;
  }
  if (nsup > 0)
    HIPCK(hipMemcpyAsync(out, sup, static_cast<size_t>(nsup) * nv * sizeof(double), hipMemcpyDeviceToHost,
                         ctx->stream));
  if ((rc = sync(ctx))) return rc;
  return static_cast<int>(nsup);
}

int mgicp_debug_finish_supers(mgicp_ctx* ctx, int nv, const double* rows, long long nsup, long long maxsup,
                              int nranks, double* out) {
  if (!ctx || !rows || !out || (nv != kRedVals && nv != kMomVals) || nsup < 0 || maxsup < 0 || nranks < 1)
    return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const size_t nrow = static_cast<size_t>(nranks) * maxsup * nv;
  DevBuf<double> d, o;
  HIPCK(d.reserve(std::max<size_t>(nrow, 1)));
  HIPCK(o.reserve(nv));
  if (nrow) HIPCK(hipMemcpyAsync(d.p, rows, nrow * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCK(launch_finish_supers(d.p, nsup, maxsup, nranks, nv, o.p, ctx->stream));
  HIPCK(hipMemcpyAsync(out, o.p, nv * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  int rc = sync(ctx);
  d.release();
  o.release();
  return rc;
}

int mgicp_debug_wave_reduce(mgicp_ctx* ctx, const double* in, int nwaves, double* out_tree, double* out_rs) {
  if (!ctx || !in || !out_tree || !out_rs || nwaves <= 0) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  const size_t nin = static_cast<size_t>(nwaves) * 64 * 16, nout = static_cast<size_t>(nwaves) * 16;
  DevBuf<double> d, t, r;
  HIPCK(d.reserve(nin));
  HIPCK(t.reserve(nout));
  HIPCK(r.reserve(nout));
  HIPCK(hipMemcpyAsync(d.p, in, nin * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCK(launch_wave_reduce_check(d.p, nwaves, t.p, r.p, ctx->stream));
  HIPCK(hipMemcpyAsync(out_tree, t.p, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCK(hipMemcpyAsync(out_rs, r.p, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  int rc = sync(ctx);
  d.release();
  t.release();
  r.release();
  return rc;
}

int mgicp_debug_trace(mgicp_ctx* ctx, float* out, int max_iters) {
  if (!ctx || !out || max_iters < 0) return MGICP_E_INVALID;
  const int n = static_cast<int>(ctx->trace.size() / 16);
  const int m = std::min(n, max_iters);
  std::memcpy(out, ctx->trace.data(), static_cast<size_t>(m) * 16 * sizeof(float));
  return n;
}

int mgicp_debug_kernel_times(mgicp_ctx* ctx, double out_ms[MGICP_KERNEL_FAMILIES],
                             int out_counts[MGICP_KERNEL_FAMILIES]) {
  if (!ctx || !out_ms) return MGICP_E_INVALID;
  prof_resolve(ctx);
  for (int i = 0; i < kFams; ++i) {
    out_ms[i] = ctx->fam_cnt[i] ? ctx->fam_ms[i] / ctx->fam_cnt[i] : 0.0;
    if (out_counts) out_counts[i] = ctx->fam_cnt[i];
  }
  return MGICP_OK;
}

int mgicp_set_profiling(mgicp_ctx* ctx, int on) {
  if (!ctx) return MGICP_E_INVALID;
  (void)hipSetDevice(ctx->device);
  cancel_gated(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  srv_release(ctx);
  prof_resolve(ctx);
  ctx->profiling = on != 0;
  ctx->prof_tick = 0;
  for (int i = 0; i < kFams; ++i) {
    ctx->fam_ms[i] = 0;
    ctx->fam_cnt[i] = 0;
  }
  return MGICP_OK;
}

// r05 target cache: [0] the current target was adopted from the cache, [1] adoptions and [2] donations
// on this device so far (process-wide), [3] an entry is cached on this device, [4] the source grid's start
// from the cached target's cell size (r05; since r06 always 0: the source's grid never depends on the target)
int mgicp_debug_cache_stats(mgicp_ctx* ctx, long long out[5]) {
  if (!ctx || !out) return MGICP_E_INVALID;
  TargetCache& c = g_tcache[ctx->device & 63];
  std::lock_guard<std::mutex> lk(c.mu);
  out[0] = ctx->tcache_adopted ? 1 : 0;
  out[1] = c.hits;
  out[2] = c.donations;
  out[3] = c.valid ? 1 : 0;
  out[4] = 0;  // r06: no speculative source grid any more (the source's grid never depends on the target)
  return MGICP_OK;
}

int mgicp_debug_match_stats(mgicp_ctx* ctx, long long out[8]) {
  if (!ctx || !out) return MGICP_E_INVALID;
  std::copy(ctx->match_stats, ctx->match_stats + 8, out);
  return MGICP_OK;
}

// Test / diagnostic forms of the engine (INTEGRATION.md "Debug options"): explicit per-context calls,
// never environment variables, so a deployment cannot switch a kernel by accident.
// Pending covariance launches are joined and the stream drained first; list-related options drop the
// target's 1-NN cell lists.
int mgicp_debug_option(mgicp_ctx* ctx, const char* name, double value) {
  if (!ctx || !name) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = cov_join_all(ctx);
  if (rc || (rc = sync(ctx))) return rc;
  const std::string n(name);
  const bool on = value != 0.0;
  const int iv = static_cast<int>(value);
  if (n == "resident") ctx->resident = on;              // resident pass server (else one launch per pass)
  else if (n == "host_rows") ctx->host_rows = on;       // server supers as stamped host rows (else device total)
  else if (n == "srv_cus") ctx->srv_cus = std::max(0, iv);  // cap on the server's blocks (0 = every CU)
  else if (n == "fused_finish") ctx->fused_finish = on; // in-launch reduction finish of launched passes
  else if (n == "gated") ctx->gated = on;               // launched passes pre-queued behind a command gate
  else if (n == "pass_memo") ctx->pass_memo = on;       // no pass at a transform the BFGS run has passed over (else one per new x)
  else if (n == "async_cov") ctx->async_tgt = on && ctx->aux_stream;  // set_*'s covariance head start
  else if (n == "lazy_src_cov") {                       // source covariances of accepted points only
    ctx->lazy_src_cov = on;
    ctx->src.have_cov = false;
    ctx->src_lazy_ready = false;
  } else if (n == "knn_wave") {                         // k-NN: lazy pass + hand-offs one wave per point (1) or per lane (0)
    ctx->knn_wave = on;
  } else if (n == "knn_logged") {                       // k-NN: the logged kernel + hand-off (1) or the register-list kernel only (0)
    ctx->knn_logged = on;
    ctx->src.have_cov = ctx->tgt.have_cov = false;
    ctx->src_lazy_ready = false;
  } else if (n == "vlist") ctx->vlist = on, ctx->vl_valid = false;  // the target's 1-NN cell lists
  else if (n == "vlist_cold") ctx->vl_cold_groups = std::max(0, iv), ctx->vl_valid = false;
  else if (n == "vlist_eager") ctx->vl_eager = on, ctx->vl_valid = false;
  else if (n == "vlist_pool") {                         // list pool of max(N, 4096) entries (0: the default size)
    ctx->vl_pool_entries = value >= 1.0 ? static_cast<size_t>(std::min(value, 134217728.0)) : 0;
    ctx->vl_valid = false;
  } else if (n == "vlist_stats") ctx->vl_stats = on;    // per-sweep list statistics on stderr
  else if (n == "fuse_compact") ctx->fuse_compact = on; // compaction fused into listed sweeps
  else if (n == "round_fast") ctx->round_fast = on;     // r08: a clean fused sweep ends its round (0: every follow-up launched)
  else if (n == "rows_running") ctx->rows_running = on; // r08: single rank, the row total taken while the rows land
  else if (n == "target_cache") ctx->tcache_on = on;    // adopt / leave the target state (process cache)
  else if (n == "match_pairs_per_launch")               // mgicp_match_features: pairs of one launch (0: the default)
    ctx->match_pairs_per_launch = value >= 1.0 ? static_cast<unsigned long long>(std::min(value, 9.0e18)) : kMatchPairsPerLaunch;
  else if (n == "ransac_batch")                         // mgicp_reject_ransac: hypotheses of one launch (0: the default)
    ctx->ransac_batch = iv >= 1 ? std::min(iv, kRansacBatch) : kRansacBatch;
  else if (n == "nc_small_limit")                       // mgicp_normal_clusters: records above which a round goes wide (0: the default)
    ctx->nc_small_limit = iv >= 1 ? std::min(iv, static_cast<int>(kNcSmallCap)) : static_cast<int>(kNcSmallLimit);
  else if (n == "bar_cmd") {                            // server commands through the BAR (else pinned copy)
    ctx->bar = on;
    if (!on && ctx->bar_cmd) {
      (void)hipFree(ctx->bar_cmd);
      ctx->bar_cmd = nullptr;
    }
    if (on && !ctx->bar_cmd) {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.isLargeBar &&
          hipExtMallocWithFlags(reinterpret_cast<void**>(&ctx->bar_cmd), sizeof(PassCmd), hipDeviceMallocFinegrained) ==
              hipSuccess)
        HIPCK(hipMemset(ctx->bar_cmd, 0, sizeof(PassCmd)));
      else
        ctx->bar_cmd = nullptr;
    }
  } else {
    return fail(ctx, MGICP_E_INVALID, "unknown debug option: " + n);
  }
  return MGICP_OK;
}

}  // extern "C"
