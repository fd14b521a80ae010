// mgicp_pass.hip -- the objective passes of a BFGS run and their transport: the command block of the
// resident server and of the gated passes, the host rows (private or the node-wide segment), the waits,
// the take-over, the RCCL combine, and DeviceFunctor (OptimizationFunctorWithIndices::fdf on the
// device), which chooses a delivery path per pass and calls it.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mgicp_ctx.hpp"

using namespace mgicp;

namespace {

// One resident server per device and process: its blocks need every CU of the device (one block
// per CU, 512 registers per lane), so a second context aligning on the same device at the same
// time runs launched passes instead of a second server.
std::atomic<int> g_srv_busy[64];

// GICP::applyState(t = I, x): R = AngleAxisf(x5,Z) * AngleAxisf(x4,Y) * AngleAxisf(x3,X)
// evaluated through Eigen's quaternion products, then t.col(3) += (x0, x1, x2, 0).
struct Quat { float w, x, y, z; };
// r06: glibc's sincosf / sincos, not sinf + cosf / sin + cos.  PCL is built by gcc, whose sincos pass
// turns Eigen's cos(ha) / sin(ha) (and computeRDerivative's cos / sin of each angle) into ONE sincos call;
// glibc's sincos differs from separate sin / cos calls by an ulp on rare arguments (7 in 1e5 random
// gradients differed, tests/test_parity_configs_gpu.py::test_oracle_on_the_engine_tree_is_bitwise_the_engine
// caught one), and clang never forms it -- so the engine names it.
Quat quat_axis(float angle, int axis) {
  const float ha = 0.5f * angle;
  float s, c;
  ::sincosf(ha, &s, &c);
  Quat q{c, 0.f, 0.f, 0.f};
  if (axis == 0) q.x = s;
  if (axis == 1) q.y = s;
  if (axis == 2) q.z = s;
  return q;
}
Quat quat_mul(const Quat& a, const Quat& b) {
  Quat r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
  r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
  return r;
}

// GICP::computeRDerivative + matricesInnerProd (tr(dR * Rsum))
void r_derivative(const Vec6& x, const double R[3][3], Vec6& g) {
  const double phi = x[3], theta = x[4], psi = x[5];
  double cphi, sphi, ctheta, stheta, cpsi, spsi;  // glibc's sincos, as gcc-built PCL calls it (quat_axis)
  ::sincos(phi, &sphi, &cphi);
  ::sincos(theta, &stheta, &ctheta);
  ::sincos(psi, &spsi, &cpsi);
  double d[3][3][3];
  // d/dphi
  d[0][0][0] = 0.; d[0][1][0] = 0.; d[0][2][0] = 0.;
  d[0][0][1] = sphi * spsi + cphi * cpsi * stheta;
  d[0][1][1] = -cpsi * sphi + cphi * spsi * stheta;
  d[0][2][1] = cphi * ctheta;
  d[0][0][2] = cphi * spsi - cpsi * sphi * stheta;
  d[0][1][2] = -cphi * cpsi - sphi * spsi * stheta;
  d[0][2][2] = -ctheta * sphi;
  // d/dtheta
  d[1][0][0] = -cpsi * stheta;
  d[1][1][0] = -spsi * stheta;
  d[1][2][0] = -ctheta;
  d[1][0][1] = cpsi * ctheta * sphi;
  d[1][1][1] = ctheta * sphi * spsi;
  d[1][2][1] = -sphi * stheta;
  d[1][0][2] = cphi * cpsi * ctheta;
  d[1][1][2] = cphi * ctheta * spsi;
  d[1][2][2] = -cphi * stheta;
  // d/dpsi
  d[2][0][0] = -ctheta * spsi;
  d[2][1][0] = cpsi * ctheta;
  d[2][2][0] = 0.;
  d[2][0][1] = -cphi * cpsi - sphi * spsi * stheta;
  d[2][1][1] = -cphi * spsi + cpsi * sphi * stheta;
  d[2][2][1] = 0.;
  d[2][0][2] = cpsi * sphi - cphi * spsi * stheta;
  d[2][1][2] = sphi * spsi + cphi * cpsi * stheta;
  d[2][2][2] = 0.;
  for (int a = 0; a < 3; ++a) {
    double r = 0.;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r += d[a][j][i] * R[i][j];
    g[3 + a] = r;
  }
}

// command block of the queued gated pass: op / reverse / A first, then the sequence number
void publish_cmd(mgicp_ctx* ctx, unsigned long long seq, unsigned int op, int reverse, const Xf34* A,
                 unsigned int rstamp = 0) {
  // every 8-byte half: (stamp << 32) | word, one aligned 8-byte store each (single-copy atomic)
  unsigned int w[kCmdWords] = {};
  if (A) std::memcpy(w, A->m, 12 * sizeof(unsigned int));
  w[12] = op;
  w[13] = static_cast<unsigned int>(reverse);
  w[14] = rstamp;
  const unsigned long long stamp = static_cast<unsigned long long>(static_cast<unsigned int>(seq)) << 32;
  if (ctx->bar_cmd) {
    // device memory through the BAR: aligned 8-byte stores, then a store fence so they leave the
    // core's write-combining buffers now
    volatile unsigned long long* b = ctx->bar_cmd->h;
    for (int i = 0; i < kCmdWords; ++i) b[i] = stamp | w[i];
    __builtin_ia32_sfence();
  }
  for (int i = 0; i < kCmdWords; ++i) __atomic_store_n(&ctx->h_cmd->h[i], stamp | w[i], __ATOMIC_RELEASE);
}

// Wait for pass `seq` to publish its sums: spin on the mapped completion word; after ~0.5 s fall
// back to a stream synchronisation so a failed launch surfaces as an error instead of a hang.
int wait_pass(mgicp_ctx* ctx, unsigned long long seq) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(ctx->h_flag, __ATOMIC_ACQUIRE) == seq) return MGICP_OK;
    if ((spins & 1023u) == 1023u &&
        std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500))
      break;
  }
  int rc = sync(ctx);
  if (rc) return rc;
  if (__atomic_load_n(ctx->h_flag, __ATOMIC_ACQUIRE) != seq)
    return fail(ctx, MGICP_E_HIP, "objective pass finished without publishing its sums");
  return MGICP_OK;
}

// r05 xGMI: the pass total the rank's totaler stored (every rank's rows arrived in its buffer)
int wait_xtot(mgicp_ctx* ctx, unsigned int rstamp, double out[kRedVals]) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t* row = reinterpret_cast<const uint64_t*>(ctx->h_xtot);
  for (unsigned spins = 0; !shm::row_complete(row, rstamp); ++spins) {
    if ((spins & 1023u) == 1023u && shm::elapsed_s(t0) > ctx->remote_deadline_s)
      return fail(ctx, MGICP_E_COMM, "xGMI row exchange: the pass total did not complete (a rank stopped publishing)");
  }
  shm::row_decode(row, out);
  return MGICP_OK;
}

// A server pass missed its deadline (its blocks could not all run: other work on the device, a
// profiler, a withheld block in the tests): cancel the server -- blocks still waiting see the later
// command and exit, blocks that start late exit at their first gate -- and re-run the pass as a
// launched kernel that writes the same rows with the same stamp (the sums are bitwise those of the
// server: same chunks, lane order and tree).  The rest of the align runs launched passes.
int take_over(mgicp_ctx* ctx, unsigned int rstamp, const Xf34& A) {
  cancel_gated(ctx);  // tickets re-armed on the stream after the server has exited
  ctx->srv_degraded = true;
  ctx->st[kStTakeover]++;
  ctx->st[kStLaunchedPass]++;
  const size_t ns = ctx->shard_p1() - ctx->shard_p0();
  HIPCK(launch_fdf_soa(corr_soa(ctx), ctx->ccnt.p, ns, A, ctx->partial.p, ctx->spart.p,
                       fdf_grid_blocks(ns, kFdfMaxBlocks), ctx->tickets.p, nullptr, 0, nullptr, 0, ctx->stream,
                       row_view(ctx).dev_rows(rstamp), rstamp));
  // host-row passes leave the tickets as multiples of their supers' sizes: re-arm them for whatever
  // form the next pass takes
  HIPCK(hipMemsetAsync(ctx->tickets.p, 0, ctx->tickets_n * sizeof(unsigned int), ctx->stream));
  return MGICP_OK;
}

// totals (nv values) of the shard's super partials `sup`: all-gathered across ranks over RCCL and
// finished in the fixed global order (launch_finish_supers), or -- single rank or detached shard
// -- finished over this shard's own supers
int combine_supers(mgicp_ctx* ctx, int nv, const double* sup, double* out) {
  if (ctx->comm) {
    const long long msup = ctx->max_supers();
    HIPCK(ctx->gath.reserve(static_cast<size_t>(ctx->nranks) * msup * nv));
    NCCLCK(ncclAllGather(sup, ctx->gath.p, static_cast<size_t>(msup) * nv, ncclDouble, ctx->comm, ctx->stream));
    HIPCK(launch_finish_supers(ctx->gath.p, ctx->nsup_total(), msup, ctx->nranks, nv, out, ctx->stream));
  } else {
    const long long ns = ctx->nsup_local();
    HIPCK(launch_finish_supers(sup, ns, ns, 1, nv, out, ctx->stream));
  }
  return MGICP_OK;
}

// Host timers of the MGICP_PASS_DIAG builds (ensure_host_red allocates h_ptimes / h_gtrace there;
// report_pass_times prints them at the end of an align).  No-ops while the pointer is null.
inline double ptimes_now(const mgicp_ctx* ctx) { return ctx->h_ptimes ? now_ms() : 0.0; }
// a server pass is about to be published: host turnaround since the previous pass's rows; returns now
inline double ptimes_publish(mgicp_ctx* ctx, double t_entry) {
  const double t_pub = ptimes_now(ctx);
  if (ctx->h_ptimes && ctx->ht_last_rows > 0 && t_pub - ctx->ht_last_rows < 1.0) {
    ctx->ht_host += t_pub - ctx->ht_last_rows;
    ctx->ht_bfgs += t_entry - ctx->ht_last_rows;
    ++ctx->ht_nh;
  }
  return t_pub;
}
inline void ptimes_rows(mgicp_ctx* ctx, double t_pub) {  // the rows of the pass published at t_pub are complete
  if (!ctx->h_ptimes) return;
  ctx->ht_last_rows = now_ms();
  ctx->ht_dev += ctx->ht_last_rows - t_pub;
  ++ctx->ht_n;
}
inline void ptimes_eval(mgicp_ctx* ctx) {  // f, g of the pass whose rows completed last are ready
  if (!ctx->h_ptimes || !(ctx->ht_last_rows > 0)) return;
  ctx->ht_eval += now_ms() - ctx->ht_last_rows;
  ++ctx->ht_ne;
}
inline void gtrace_mark(mgicp_ctx* ctx, unsigned long long slot) {  // host wall clock (us) of a gated pass's event
  if (ctx->h_gtrace) ctx->host_gt[slot] = now_ms() * 1e3;
}

// One objective pass as its delivery paths see it
struct PassArgs {
  unsigned long long seq;  // the pass's sequence number (completion word, command block)
  unsigned int rstamp;     // its row stamp
  Xf34 Ax;                 // the state's transform
  size_t ns;               // points of this rank's shard
  // alternate the sweep direction so each pass starts on the Infinity-Cache-resident tail
  // of the previous one (deterministic: the sums do not depend on the direction): 360 MB of
  // streams at 5M points exceed the 256 MiB Infinity Cache (73 -> 68 us per pass)
  int reverse;
};

// How a pass is delivered.  Single GPU: the finishing wave writes the totals straight into mapped
// pinned host memory (inlaunch).  Shared row segment (any rank count): every pass -- server or launched
// -- writes its super rows there and every host takes the total.  Otherwise (RCCL only) the pass leaves
// its super partials, then combine_supers (RCCL all-gather + the fixed-order total) and a one-wave
// kernel publishes the totals plus the completion word.
struct PassPlan {
  bool inlaunch = false;  // the pass's finishing wave publishes the totals itself
  bool gate = false;      // launched passes pre-queue their successor behind the command block
  bool rows = false;      // the sums travel as stamped host rows
  int nsrv = 0;           // blocks of the resident server (0: a launched pass)
};

int plan_pass(mgicp_ctx* ctx, size_t ns, PassPlan& pl) {
  const bool shm_rows = ctx->have_shm;
  pl.inlaunch = ctx->fused_finish && !ctx->comm && ctx->nranks == 1 && !shm_rows;
  pl.gate = ctx->gated && pl.inlaunch && !ctx->profiling;
  const bool want_srv = ctx->resident && !ctx->srv_degraded && !ctx->profiling && (pl.gate || shm_rows);
  int cap = ctx->srv_cus > 0 ? std::min(ctx->srv_cus, ctx->cus) : ctx->cus;
  if (ctx->have_xgmi) cap = std::min(cap, ctx->cus - 1);  // one CU left to the totaler wave
  pl.nsrv = want_srv ? fdf_server_blocks(ns, cap) : 0;
  // the host rows first: a failure here (e.g. a source larger than the shared segment) must not
  // leave the device's server slot taken
  int rc;
  if (!ctx->srv_live && (shm_rows || (pl.nsrv > 0 && ctx->host_rows)) && (rc = ensure_rows(ctx))) return rc;
  if (pl.nsrv > 0 && !ctx->srv_live && !ctx->srv_locked) {
    int idle = 0;  // one server per device and process (g_srv_busy)
    ctx->srv_locked = g_srv_busy[ctx->device & 63].compare_exchange_strong(idle, 1, std::memory_order_acq_rel);
    if (!ctx->srv_locked) {
      pl.nsrv = 0;
      ctx->st[kStSrvDenied]++;
    }
  }
  pl.rows = shm_rows || (pl.nsrv > 0 && ctx->host_rows);
  if (ctx->have_xgmi && pl.nsrv <= 0)
    return fail(ctx, MGICP_E_COMM, "xGMI row exchange needs the resident pass server on every rank (the device's "
                                   "server slot is held by another context, or profiling is on)");
  return MGICP_OK;
}

// the resident server runs every pass of this BFGS run: started with the first one
int server_start(mgicp_ctx* ctx, const PassArgs& a, const PassPlan& pl) {
  cancel_gated(ctx);
  ctx->ht_last_rows = 0;  // host-view diagnostics: a new BFGS run, not a host step
  const RowView rv = row_view(ctx);
  const bool xg = ctx->have_xgmi;
  // xGMI: rows into this rank's exchange buffer and every peer's, at the global super index
  PeerRows pr{};
  unsigned long long* xr = nullptr;
  if (xg) {
    xr = ctx->xrows.p + static_cast<size_t>(rv.first) * shm::kRowWords;
    pr.n = static_cast<int>(ctx->xpeer.size());
    for (int r = 0; r < pr.n; ++r)
      pr.p[r] = static_cast<unsigned long long*>(ctx->xpeer[r]) + static_cast<size_t>(rv.first) * shm::kRowWords;
  }
  hipEvent_t ea = ev_get(ctx);
  hipError_t e = hipEventRecord(ea, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->tickets.p, 0, ctx->tickets_n * sizeof(unsigned int), ctx->stream);
  {
    ProfScope ps(ctx, kFamFdf);
    if (e == hipSuccess)
      e = launch_fdf_server(corr_soa(ctx), ctx->ccnt.p, a.ns, ctx->partial.p, ctx->spart.p, ctx->tickets.p,
                            pl.inlaunch ? ctx->d_h_red : nullptr, ctx->d_flag, a.seq,
                            ctx->bar_cmd ? ctx->bar_cmd : ctx->d_cmd, ctx->mail, ctx->gate_timeout, ctx->d_ptimes, 0,
                            a.Ax, xg ? xr : (pl.rows ? rv.dev_rows(0) : nullptr), rv.stride, pl.nsrv,
                            ctx->bar_cmd ? pl.nsrv : 1, ctx->stall_pass, ctx->tpart.p, ctx->stream, xg ? &pr : nullptr);
    // the totaler of this BFGS run (its own stream; exits on the generation change of the cancel)
    if (e == hipSuccess && xg) {
      const unsigned int gen = ++ctx->xgen;
      __atomic_store_n(ctx->h_xgen, gen, __ATOMIC_RELEASE);
      e = launch_xgmi_total(ctx->xrows.p, rv.stride, rv.ntot, a.rstamp, ctx->d_xtot, ctx->d_xgen, gen,
                            ctx->gate_timeout, ctx->xstream);
    }
  }
  hipEvent_t eb = nullptr;
  if (e == hipSuccess) {
    eb = ev_get(ctx);
    e = hipEventRecord(eb, ctx->stream);  // completes when the server exits (stream order)
  }
  if (e != hipSuccess) {
    g_srv_busy[ctx->device & 63].store(0, std::memory_order_release);
    ctx->srv_locked = false;
    ctx->pool.push_back(ea);
    if (eb) ctx->pool.push_back(eb);
    HIPCK(e);
  }
  ctx->srv_ev.push_back({ea, eb, 0});
  ctx->srv_live = true;
  ctx->st[kStSrvLaunch]++;
  ctx->st[kStBar] = ctx->bar_cmd ? 1 : 0;
  return MGICP_OK;
}

// a pass of the resident server: publish its command, then wait for the sums in the form the server
// delivers them (the xGMI totaler's row, the host rows, or the in-launch totals)
int server_pass(mgicp_ctx* ctx, const PassArgs& a, const PassPlan& pl, double t_entry, double sums[kRedVals]) {
  int rc;
  if (!ctx->srv_live && (rc = server_start(ctx, a, pl))) return rc;
  if (!ctx->srv_ev.empty()) ctx->srv_ev.back().passes++;
  const double t_pub = ptimes_publish(ctx, t_entry);
  publish_cmd(ctx, a.seq, kPassRun, 0, &a.Ax, a.rstamp);
  ctx->srv_next = a.seq + 1;
  ctx->st[kStSrvPass]++;
  if (ctx->have_xgmi) return wait_xtot(ctx, a.rstamp, sums);
  if (pl.rows) {
    if ((rc = wait_rows(ctx, a.rstamp, a.Ax, sums, true))) return rc;
    ptimes_rows(ctx, t_pub);
    return MGICP_OK;
  }
  if ((rc = wait_pass(ctx, a.seq))) return rc;
  std::memcpy(sums, ctx->h_red, kRedVals * sizeof(double));
  return MGICP_OK;
}

// a launched pass into the shared rows (profiling, a degraded align, an unservable shard)
int launched_rows_pass(mgicp_ctx* ctx, const PassArgs& a, double sums[kRedVals]) {
  cancel_gated(ctx);
  {
    ProfScope ps(ctx, kFamFdf);
    HIPCK(launch_fdf_soa(corr_soa(ctx), ctx->ccnt.p, a.ns, a.Ax, ctx->partial.p, ctx->spart.p,
                         fdf_grid_blocks(a.ns, kFdfMaxBlocks), ctx->tickets.p, nullptr, a.reverse, nullptr, a.seq,
                         ctx->stream, row_view(ctx).dev_rows(a.rstamp), a.rstamp));
  }
  return wait_rows(ctx, a.rstamp, a.Ax, sums, false);
}

// a launched pass that publishes its totals and the completion word: the resident gated pass (handed
// its state) or a fresh launch; gated, it queues its successor; not in-launch, the RCCL combine follows
int launched_pass(mgicp_ctx* ctx, const PassArgs& a, const PassPlan& pl, double sums[kRedVals]) {
  const CorrSoA c = corr_soa(ctx);
  const int nb = fdf_grid_blocks(a.ns, kFdfMaxBlocks);
  double* out = pl.inlaunch ? ctx->d_h_red : nullptr;
  int rc;
  if (ctx->gated_seq == a.seq) {
    // pass `seq` is already resident, waiting: hand it its state
    publish_cmd(ctx, a.seq, kPassRun, a.reverse, &a.Ax);
    gtrace_mark(ctx, 2 * (a.seq & 1023) + 1);
    ctx->gated_seq = 0;
  } else {
    cancel_gated(ctx);
    ProfScope ps(ctx, kFamFdf);
    HIPCK(launch_fdf_soa(c, ctx->ccnt.p, a.ns, a.Ax, ctx->partial.p, ctx->spart.p, nb,
                         ctx->tickets.p, out, a.reverse, pl.inlaunch ? ctx->d_flag : nullptr, a.seq,
                         ctx->stream));
  }
  if (pl.gate) {
    // blocks polling the host copy of the command: 1 measured best (14.15 ms / C4 align; 8 pollers
    // 14.8 ms, all 256 blocks on host memory ~70 ms: PCIe read contention; profiles/r02/ab_gate)
    constexpr int kGatePollers = 1;
    // queue pass seq + 1 now (its launch overlaps this pass); it runs once the BFGS step has
    // published x_{k+1}, or exits on cancel when the BFGS run ends
    HIPCK(launch_fdf_soa_gated(c, ctx->ccnt.p, a.ns, ctx->partial.p, ctx->spart.p, nb,
                               ctx->tickets.p, out, ctx->d_flag, a.seq + 1, ctx->d_cmd, ctx->mail,
                               ctx->gate_timeout, ctx->d_gtrace, kGatePollers, ctx->stream));
    ctx->gated_seq = a.seq + 1;
  }
  if (!pl.inlaunch) {
    {
      ProfScope ps(ctx, kFamRed);
      if ((rc = combine_supers(ctx, kRedVals, ctx->spart.p, ctx->red.p))) return rc;
    }
    HIPCK(launch_publish(ctx->red.p, kRedVals, ctx->d_h_red, ctx->d_flag, a.seq, ctx->stream));
  }
  rc = wait_pass(ctx, a.seq);
  gtrace_mark(ctx, 2 * ((a.seq + 1) & 1023));  // sums of seq seen
  if (rc) return rc;
  std::memcpy(sums, ctx->h_red, kRedVals * sizeof(double));
  return MGICP_OK;
}

}  // namespace

Mat4 mgicp::apply_state(const Vec6& x) {
  const Quat q = quat_mul(quat_mul(quat_axis(static_cast<float>(x[5]), 2),
                                   quat_axis(static_cast<float>(x[4]), 1)),
                          quat_axis(static_cast<float>(x[3]), 0));
  const float tx = 2.0f * q.x, ty = 2.0f * q.y, tz = 2.0f * q.z;
  const float twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const float txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const float tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  Mat4 T = Mat4::identity();
  T.m[0][0] = 1.0f - (tyy + tzz);
  T.m[0][1] = txy - twz;
  T.m[0][2] = txz + twy;
  T.m[1][0] = txy + twz;
  T.m[1][1] = 1.0f - (txx + tzz);
  T.m[1][2] = tyz - twx;
  T.m[2][0] = txz - twy;
  T.m[2][1] = tyz + twx;
  T.m[2][2] = 1.0f - (txx + tyy);
  T.m[0][3] = 0.0f + static_cast<float>(x[0]);
  T.m[1][3] = 0.0f + static_cast<float>(x[1]);
  T.m[2][3] = 0.0f + static_cast<float>(x[2]);
  return T;
}

void mgicp::prof_resolve(mgicp_ctx* ctx) {
  for (auto& p : ctx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      ctx->fam_ms[p.fam] += ms;
      ctx->fam_cnt[p.fam] += 1;
    }
    ctx->pool.push_back(p.a);
    ctx->pool.push_back(p.b);
  }
  ctx->pending.clear();
}

// release a queued gated pass (or the resident server) without running it (end of a BFGS run,
// any stream drain)
void mgicp::cancel_gated(mgicp_ctx* ctx) {
  if (ctx->srv_live) {
    xgmi_cancel(ctx);
    publish_cmd(ctx, ctx->srv_next, kPassCancel, 0, nullptr);
    ctx->pass_seq = std::max(ctx->pass_seq, ctx->srv_next);  // its sequence number is spent
    ctx->srv_live = false;
    // host-row passes leave the tickets as multiples of their supers' sizes: re-arm them for the
    // launched passes (stream order: after the server has exited)
    (void)hipMemsetAsync(ctx->tickets.p, 0, ctx->tickets_n * sizeof(unsigned int), ctx->stream);
    // the device's server slot stays with this context until its stream has drained (sync): a
    // cancelled server may still be finishing, and another context's server must not start beside
    // it; this context's next BFGS run re-launches behind it in stream order
  }
  if (!ctx->gated_seq) return;
  publish_cmd(ctx, ctx->gated_seq, kPassCancel, 0, nullptr);
  ctx->pass_seq = std::max(ctx->pass_seq, ctx->gated_seq);  // its sequence number is spent
  ctx->gated_seq = 0;
}

// server launches whose events have completed (after a drain: all of them) -> the in-align totals
void mgicp::srv_resolve(mgicp_ctx* ctx) {
  for (auto& e : ctx->srv_ev) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      ctx->srv_time_ms += ms;
      ctx->srv_time_passes += e.passes;
      ctx->srv_time_launches += 1;
    }
    ctx->pool.push_back(e.a);
    ctx->pool.push_back(e.b);
  }
  ctx->srv_ev.clear();
}

// after a stream drain: no server of this context is running, the device's slot is free again
void mgicp::srv_release(mgicp_ctx* ctx) {
  if (ctx->srv_locked && !ctx->srv_live) {
    g_srv_busy[ctx->device & 63].store(0, std::memory_order_release);
    ctx->srv_locked = false;
  }
}

int mgicp::sync(mgicp_ctx* ctx) {
  cancel_gated(ctx);  // a queued gated pass would otherwise hold the stream until its timeout
  HIPCK(hipStreamSynchronize(ctx->stream));
  srv_release(ctx);
  if (ctx->profiling) prof_resolve(ctx);
  if (!ctx->srv_ev.empty()) srv_resolve(ctx);
  return MGICP_OK;
}

// Row stamps count objective passes; every buffer that holds stamps of earlier passes (the server's
// stamped chunk partials, this context's private host rows) is cleared whenever the count restarts
// (an attach or detach of the shared segment, the 2^31 wrap), so a stale word can never carry the
// stamp of a new pass.  The stream is drained first: no server still writes them.
int mgicp::reset_stamps(mgicp_ctx* ctx) {
  int rc = sync(ctx);
  if (rc) return rc;
  if (ctx->tpart.p && ctx->tpart_n) {
    HIPCK(hipMemsetAsync(ctx->tpart.p, 0xff, ctx->tpart_n * sizeof(unsigned long long), ctx->stream));
    HIPCK(hipStreamSynchronize(ctx->stream));
  }
  if (ctx->h_rows) std::memset(ctx->h_rows, 0, 2 * ctx->rows_cap * shm::kRowWords * sizeof(unsigned long long));
  if (ctx->have_xgmi) {  // stamps restart: no stale row of the exchange buffer may validate
    if (ctx->xstream) HIPCK(hipStreamSynchronize(ctx->xstream));
    HIPCK(hipMemsetAsync(ctx->xrows.p, 0, ctx->xrows.cap * sizeof(unsigned long long), ctx->stream));
    HIPCK(hipStreamSynchronize(ctx->stream));
    std::memset(ctx->h_xtot, 0, shm::kRowWords * sizeof(unsigned long long));
  }
  ctx->pass_idx = 0;
  ctx->gather_idx = 0;
  return MGICP_OK;
}

int mgicp::ensure_host_red(mgicp_ctx* ctx) {
  if (!ctx->h_cmd) {
    HIPCK(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_cmd), sizeof(PassCmd),
                        hipHostMallocMapped | hipHostMallocCoherent));
    HIPCK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_cmd), ctx->h_cmd, 0));
    std::memset(ctx->h_cmd, 0, sizeof(PassCmd));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0)
      khz = 100000;  // 100 MHz: the gfx9 constant wall clock
    ctx->gate_timeout = static_cast<unsigned long long>(khz) * 1000ull * 10ull;  // 10 s
    HIPCK(hipMalloc(reinterpret_cast<void**>(&ctx->mail), sizeof(PassCmd)));
    HIPCK(hipMemsetAsync(ctx->mail, 0, sizeof(PassCmd), ctx->stream));
    // host stores into device memory need the whole VRAM behind the PCIe BAR (large BAR); without
    // it block 0 polls the pinned copy
    hipDeviceProp_t prop;
    const bool large_bar = hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.isLargeBar;
    if (ctx->bar && large_bar && !ctx->bar_cmd) {
      if (hipExtMallocWithFlags(reinterpret_cast<void**>(&ctx->bar_cmd), sizeof(PassCmd), hipDeviceMallocFinegrained) !=
          hipSuccess)
        ctx->bar_cmd = nullptr;  // no host-writable device memory: block 0 polls the pinned copy
      else
        HIPCK(hipMemset(ctx->bar_cmd, 0, sizeof(PassCmd)));  // complete before the host's first store
    }
#if MGICP_PASS_DIAG
    // diagnostic builds (make variant DEFS=-DMGICP_PASS_DIAG=1): per-pass device / host timestamps of
    // the resident server and of the gated passes, summarised on stderr at the end of every align
    {
      HIPCK(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_ptimes), 2 * 1024 * sizeof(unsigned long long),
                          hipHostMallocMapped | hipHostMallocCoherent));
      HIPCK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_ptimes), ctx->h_ptimes, 0));
      std::memset(ctx->h_ptimes, 0, 2 * 1024 * sizeof(unsigned long long));
    }
    {
      HIPCK(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_gtrace), 4 * 1024 * sizeof(unsigned long long),
                          hipHostMallocMapped | hipHostMallocCoherent));
      HIPCK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_gtrace), ctx->h_gtrace, 0));
      std::memset(ctx->h_gtrace, 0, 4 * 1024 * sizeof(unsigned long long));
      ctx->host_gt.assign(2 * 1024, 0.0);
    }
#endif
  }
  if (!ctx->h_round) {  // r08: the listed sweep's verdict words (stamp 0 is never a round's stamp)
    HIPCK(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_round), 8 * sizeof(unsigned long long),
                        hipHostMallocMapped | hipHostMallocCoherent));
    HIPCK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_round), ctx->h_round, 0));
    std::memset(ctx->h_round, 0, 8 * sizeof(unsigned long long));
  }
  if (ctx->h_red) return MGICP_OK;
  // kRedVals sums followed by the pass-completion word (see launch_fdf_soa's done_flag)
  HIPCK(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_red), 2 * kRedVals * sizeof(double),
                      hipHostMallocMapped | hipHostMallocCoherent));
  HIPCK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_h_red), ctx->h_red, 0));
  std::memset(ctx->h_red, 0, 2 * kRedVals * sizeof(double));
  ctx->h_flag = reinterpret_cast<unsigned long long*>(ctx->h_red + kRedVals);
  ctx->d_flag = reinterpret_cast<unsigned long long*>(ctx->d_h_red + kRedVals);
  return MGICP_OK;
}

RowView mgicp::row_view(const mgicp_ctx* ctx) {
  RowView v;
  if (ctx->have_shm) {
    v.h0 = reinterpret_cast<unsigned long long*>(ctx->shm.rows(0));
    v.d0 = reinterpret_cast<unsigned long long*>(ctx->shm_d + ctx->shm.rows_offset_bytes());
    v.stride = ctx->shm.rows_stride_words();
    v.ntot = ctx->nsup_total();
    v.first = super_first(ctx->rank, v.ntot, ctx->nranks);
    v.nloc = ctx->nsup_local();
  } else {
    v.h0 = ctx->h_rows;
    v.d0 = ctx->d_rows;
    v.stride = ctx->rows_cap * shm::kRowWords;
    v.ntot = v.nloc = ctx->nsup_local();
  }
  return v;
}

// Host rows for the current source cloud: the private buffers grow as needed (two parity buffers);
// the shared segment was sized at attach time.
int mgicp::ensure_rows(mgicp_ctx* ctx) {
  const long long nsup = ctx->nsup_total();
  if (ctx->have_shm) {
    if (nsup > ctx->shm.max_sup)
      return fail(ctx, MGICP_E_INVALID, "source cloud larger than the shared row segment (mgicp_comm_attach_shm "
                                        "max_source_points)");
    return MGICP_OK;
  }
  if (ctx->h_rows && ctx->rows_cap >= static_cast<size_t>(nsup)) return MGICP_OK;
  if (ctx->h_rows) {
    int rc = sync(ctx);  // no server of an earlier run may still hold the old rows
    if (rc) return rc;
    HIPCK(hipHostFree(ctx->h_rows));
  }
  ctx->h_rows = nullptr;
  const size_t cap = static_cast<size_t>(std::max<long long>(nsup, 64));
  const size_t bytes = 2 * cap * shm::kRowWords * sizeof(unsigned long long);
  HIPCK(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_rows), bytes, hipHostMallocMapped | hipHostMallocCoherent));
  HIPCK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_rows), ctx->h_rows, 0));
  std::memset(ctx->h_rows, 0, bytes);  // stamp 0 is never a pass's stamp
  ctx->rows_cap = cap;
  ctx->st[kStRowsAlloc]++;
  return MGICP_OK;
}

// Wait for every host row of the pass stamped rstamp (32 stamped words per super: this rank's own
// rows first, then the other ranks'), then take the total exactly as wave_total / wave_sum would on
// one wave (shm::fixed_total).  Own rows missing after row_deadline_ms: the pass is taken over
// (take_over, when allowed) and waited for again; after a stream drain every row is checked once
// more before an error is returned.  Other ranks' rows: remote_deadline_s.
int mgicp::wait_rows(mgicp_ctx* ctx, unsigned int rstamp, const Xf34& A, double out[kRedVals], bool allow_takeover) {
  const RowView rv = row_view(ctx);
  const unsigned long long* buf = rv.h0 + (rstamp & 1u) * rv.stride;
  ctx->row_sums.resize(static_cast<size_t>(std::max<long long>(rv.ntot, 1)) * kRedVals);
  auto t0 = std::chrono::steady_clock::now();
  bool taken = false;
  const double dl_own = ctx->row_deadline_ms * 1e-3;
  auto wait_row = [&](long long r, bool own) -> int {
    const unsigned long long* row = buf + shm::kRowWords * static_cast<size_t>(r);
    for (unsigned spins = 0; !shm::row_complete(reinterpret_cast<const uint64_t*>(row), rstamp); ++spins) {
      if ((spins & 1023u) != 1023u) continue;
      const double el = shm::elapsed_s(t0);
      if (own && !taken && allow_takeover && el > dl_own) {
        int rc = take_over(ctx, rstamp, A);
        if (rc) return rc;
        taken = true;
        t0 = std::chrono::steady_clock::now();
        continue;
      }
      if (own && el > (taken ? ctx->remote_deadline_s : dl_own)) {
        int rc = sync(ctx);  // drains the stream (and cancels a live server): the rows are final now
        if (rc) return rc;
        if (shm::row_complete(reinterpret_cast<const uint64_t*>(row), rstamp)) break;
        char msg[192];
        std::snprintf(msg, sizeof(msg),
                      "objective pass finished without publishing its super rows (row %lld of %lld: stamp %08x "
                      "expected, words 0 / 31 carry %08x / %08x)",
                      r, rv.nloc, rstamp, static_cast<unsigned int>(row[0] >> 32),
                      static_cast<unsigned int>(row[31] >> 32));
        return fail(ctx, MGICP_E_HIP, msg);
      }
      if (!own && el > ctx->remote_deadline_s)
        return fail(ctx, MGICP_E_COMM, "another rank did not publish its super rows (shared row segment)");
    }
    shm::row_decode(reinterpret_cast<const uint64_t*>(row), &ctx->row_sums[static_cast<size_t>(r) * kRedVals]);
    return MGICP_OK;
  };
  // r08, single rank: the lanes' sums are taken while the later rows are still on their way (rows are
  // waited for in index order, which is the order fixed_total adds them in); any other row view keeps
  // fixed_total
  static_assert(shm::RunningTotal::kVals == kRedVals, "RunningTotal restates the pass's value count");
  const bool running = ctx->rows_running && rv.first == 0 && rv.nloc == rv.ntot;
  shm::RunningTotal rt;
  if (running) rt.reset();
  for (long long r = rv.first; r < rv.first + rv.nloc; ++r) {
    int rc = wait_row(r, true);
    if (rc) return rc;
    if (running) rt.add_row(r, &ctx->row_sums[static_cast<size_t>(r) * kRedVals]);
  }
  if (running) {
    rt.finish(out);
    return MGICP_OK;
  }
  t0 = std::chrono::steady_clock::now();
  for (long long r = 0; r < rv.ntot; ++r) {
    if (r >= rv.first && r < rv.first + rv.nloc) continue;
    int rc = wait_row(r, false);
    if (rc) return rc;
  }
  shm::fixed_total(ctx->row_sums.data(), rv.ntot, kRedVals, out);
  return MGICP_OK;
}

int mgicp::ensure_iter_buffers(mgicp_ctx* ctx) {
  const size_t ns = ctx->shard_p1() - ctx->shard_p0();
  const size_t nch = static_cast<size_t>(chunk_count(ns));
  const size_t msup = static_cast<size_t>(ctx->max_supers());
  HIPCK(ctx->partial.reserve(std::max<size_t>(nch, 1) * kRedVals));
  if (ctx->tpart_n < std::max<size_t>(nch, 1) * 32) {  // stamps 0xffffffff: never a pass's stamp
    HIPCK(ctx->tpart.reserve(std::max<size_t>(nch, 1) * 32));
    HIPCK(hipMemsetAsync(ctx->tpart.p, 0xff, ctx->tpart.cap * sizeof(unsigned long long), ctx->stream));
    ctx->tpart_n = ctx->tpart.cap;
  }
  HIPCK(ctx->spart.reserve(std::max<size_t>(msup, 1) * kRedVals));
  HIPCK(ctx->ccnt.reserve(std::max<size_t>(nch, 1)));
  HIPCK(ctx->red.reserve(kRedVals));
  if (ctx->tickets_n < msup + 1) {  // zero between passes: every finishing wave re-arms its own
    HIPCK(ctx->tickets.reserve(msup + 1));
    HIPCK(hipMemsetAsync(ctx->tickets.p, 0, (msup + 1) * sizeof(unsigned int), ctx->stream));
    ctx->tickets_n = msup + 1;
  }
  int rc = ensure_host_red(ctx);
  if (rc) return rc;
  // fixed slots: chunk c's run starts at c * kChunkPts (padded to a multiple of 4 within the chunk)
  const size_t cap = std::max<size_t>(nch, 1) * kChunkPts;
  HIPCK(ctx->prev_pos.reserve(ns + 1));
  HIPCK(ctx->flags.reserve(ns + 1));
  if (ctx->corr_cap < cap) {
    HIPCK(ctx->corr_f.reserve(6 * cap));
    HIPCK(ctx->corr_d.reserve(6 * cap));
    ctx->corr_cap = cap;
  }
  return MGICP_OK;
}

// The same totals delivered to the host (GN moments once per outer iteration, fitness once per
// call).  With the shared segment: a generic gather -- this rank copies its supers to their global
// rows of the gather's parity buffer, publishes the gather index and waits for every rank's, and
// every host takes the fixed-order total itself (no collective).  Otherwise combine_supers + D2H.
int mgicp::combine_to_host(mgicp_ctx* ctx, int nv, const double* sup, double* out) {
  if (ctx->have_shm) {
    const unsigned long long g = ++ctx->gather_idx;
    double* buf = ctx->shm.gath(static_cast<int>(g & 1));
    const long long ntot = ctx->nsup_total();
    const long long first = super_first(ctx->rank, ntot, ctx->nranks), nloc = ctx->nsup_local();
    if (nloc > 0)
      HIPCK(hipMemcpyAsync(buf + static_cast<size_t>(first) * nv, sup, static_cast<size_t>(nloc) * nv * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    int rc = sync(ctx);
    if (rc) return rc;
    if (!shm::gather_publish_wait(ctx->shm, g, ctx->remote_deadline_s))
      return fail(ctx, MGICP_E_COMM, "another rank did not publish its supers (shared segment gather)");
    // the gather rows are packed nv per super: fixed_total reads rows[s * nv + v]
    shm::fixed_total(buf, ntot, nv, out);
    return MGICP_OK;
  }
  double* dst = nv == kRedVals ? ctx->red.p : ctx->mred.p;
  int rc = combine_supers(ctx, nv, sup, dst);
  if (rc) return rc;
  HIPCK(hipMemcpyAsync(ctx->h_small, dst, static_cast<size_t>(nv) * sizeof(double), hipMemcpyDeviceToHost,
                       ctx->stream));
  if ((rc = sync(ctx))) return rc;
  std::memcpy(out, ctx->h_small, static_cast<size_t>(nv) * sizeof(double));
  return MGICP_OK;
}

CorrSoA mgicp::corr_soa(mgicp_ctx* ctx) {
  const size_t c = ctx->corr_cap;
  float* f = ctx->corr_f.p;
  double* d = ctx->corr_d.p;
  return CorrSoA{f, f + c, f + 2 * c, f + 3 * c, f + 4 * c, f + 5 * c,
                 d, d + c, d + 2 * c, d + 3 * c, d + 4 * c, d + 5 * c};
}

int DeviceFunctor::pass(const Vec6& x, double sums[kRedVals]) {
  const double t_entry = ptimes_now(ctx);
  int rc;
  // the pass's row stamp: the objective-pass index, identical on every rank (0 is never a stamp;
  // stamps >= 2^31 belong to mgicp_debug_pass_bench's timing form).  At the wrap every stamped
  // buffer is cleared and the count restarts at 1, so parity buffers keep alternating.
  if (ctx->pass_idx + 1 >= 0x80000000u && (rc = reset_stamps(ctx))) return rc;
  if (ctx->quit_pass >= 0 && ctx->pass_idx + 1 >= static_cast<unsigned int>(ctx->quit_pass))
    return fail(ctx, MGICP_E_COMM, "MGICP_DEBUG_QUIT_PASS: this rank stops publishing its rows");
  PassArgs a;
  a.seq = ++ctx->pass_seq;
  a.rstamp = ++ctx->pass_idx;
  a.Ax = apply_state(x).xf();
  a.ns = ctx->shard_p1() - ctx->shard_p0();
  a.reverse = ctx->n_evals & 1;
  PassPlan pl;
  if ((rc = plan_pass(ctx, a.ns, pl))) return rc;
  if (pl.nsrv > 0) {
    rc = server_pass(ctx, a, pl, t_entry, sums);
  } else {
    ctx->st[kStLaunchedPass]++;
    rc = ctx->have_shm ? launched_rows_pass(ctx, a, sums) : launched_pass(ctx, a, pl, sums);
  }
  if (rc) return rc;
  ctx->n_evals++;
  return MGICP_OK;
}

// the sums of the pass at x -> f, g at x (the functor's memo) and the correspondence count
void DeviceFunctor::memoise(const Vec6& x, const double s[kRedVals]) {
  m = s[13];
  memo_x = x;
  memo_f = s[0] / m;
  const double sc = 2.0 / m;
  memo_g[0] = s[1] * sc;
  memo_g[1] = s[2] * sc;
  memo_g[2] = s[3] * sc;
  double R[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a][b] = s[4 + 3 * a + b] * sc;
  r_derivative(x, R, memo_g);
  have_memo = true;
}

void DeviceFunctor::remember(const Vec6& x, const double s[kRedVals]) {
  if (ctx->pass_memo) seen.insert(apply_state(x).xf().m, s);
}

int DeviceFunctor::eval(const Vec6& x, double& f, Vec6& g) {
  if (!(have_memo && std::memcmp(x.v, memo_x.v, sizeof(x.v)) == 0)) {
    // a new x whose fp32 transform this run has passed over already: the pass would return the sums
    // held (bitwise), so only f and g are taken again, g with the new x (pass_memo.hpp)
    const Xf34 A = apply_state(x).xf();
    const double* held = ctx->pass_memo ? seen.find(A.m) : nullptr;
    if (held) {
      ctx->st[kStMemoHit]++;
      memoise(x, held);
    } else {
      double s[kRedVals];
      int rc = pass(x, s);
      if (rc) return rc;
      if (ctx->pass_memo) seen.insert(A.m, s);
      memoise(x, s);
      ptimes_eval(ctx);
    }
  }
  f = memo_f;
  g = memo_g;
  return 0;
}

// DeviceFunctor for the debug entry points (mgicp_debug_fdf, mgicp_debug_fdf_sums): f and g at x, and
// the 16 raw sums of one pass at x
int mgicp::fdf_at(mgicp_ctx* ctx, const Vec6& x, double& f, Vec6& g) {
  GateGuard guard{ctx};  // no queued pass / live server outlives the call
  DeviceFunctor fn{ctx};
  return fn.eval(x, f, g);
}
int mgicp::fdf_sums_at(mgicp_ctx* ctx, const Vec6& x, double sums[kRedVals]) {
  GateGuard guard{ctx};
  DeviceFunctor fn{ctx};
  return fn.pass(x, sums);
}
int mgicp::fdf_sums_run_at(mgicp_ctx* ctx, const Vec6* xs, int n, double* sums) {
  GateGuard guard{ctx};  // the server launched by the first pass serves them all, then is cancelled
  DeviceFunctor fn{ctx};
  for (int k = 0; k < n; ++k) {
    int rc = fn.pass(xs[k], sums + static_cast<size_t>(k) * kRedVals);
    if (rc) return rc;
  }
  return MGICP_OK;
}

