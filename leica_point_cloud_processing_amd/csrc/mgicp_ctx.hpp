// mgicp_ctx.hpp -- the context and the host helpers that libmgicp.so's host translation units share:
// mgicp_engine.hip, mgicp_clouds.hip, mgicp_pass.hip, mgicp_fod.hip, mgicp_features.hip and mgicp_comm.hip (the product calls
// of include/mi355x_gicp.h, by subsystem) and mgicp_debug.hip (the test, benchmark and diagnostic calls
// of include/mi355x_gicp_debug.h).  Private: nothing here crosses the C-ABI, and the
// export map (libmgicp.map) keeps every name below out of the library's dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mi355x_gicp.h"
#include "mgicp_internal.hpp"
#include "pass_memo.hpp"
#include "pcl_bfgs.hpp"
#include "shm_rows.hpp"

using namespace mgicp;  // both including files are written inside it; struct mgicp_ctx is the C-ABI's global name

namespace mgicp {

// objective-pass launch shape over the fixed reduction tree, A/B-measured on MI355X at 5M points
// (profiles/r02/ab_tree): 512 persistent 4-wave blocks -- 2 waves per SIMD, so chunk reductions
// and tickets overlap other waves' streaming (71 us vs 76 us at 256 blocks), and the gated
// grid (134 VGPRs: 3 waves per SIMD) stays resident while it waits at the gate (14.5 ms per C4
// align vs 14.9 ms at 1024 blocks); in-launch finish
constexpr int kFdfMaxBlocks = 512;

#ifndef MGICP_PASS_DIAG
#define MGICP_PASS_DIAG 0
#endif

struct Mat4 {  // row-major float 4x4
  float m[4][4];
  static Mat4 identity() {
    Mat4 r;
    std::memset(r.m, 0, sizeof(r.m));
    r.m[0][0] = r.m[1][1] = r.m[2][2] = r.m[3][3] = 1.f;
    return r;
  }
  static Mat4 from_cm(const float* cm) {
    Mat4 r;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) r.m[i][j] = cm[j * 4 + i];
    return r;
  }
  void to_cm(float* cm) const {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) cm[j * 4 + i] = m[i][j];
  }
  bool is_identity() const {
    const Mat4 I = identity();
    return std::memcmp(m, I.m, sizeof(m)) == 0;
  }
  Xf34 xf() const {
    Xf34 x;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) x.m[4 * i + j] = m[i][j];
    return x;
  }
};

// Device buffers a reserve() replaces are freed at quiet points of their OWN context (the end of an
// align, a destroy), not at once: hipFree waits for the whole device, which stalled set_*'s grid build
// behind the other cloud's covariance head start on the second stream (r04, ~2 ms, profiles/r04/prep7).
// One graveyard per context: a context's quiet point never frees -- and so never waits
// on -- buffers of another context or device.
struct Graveyard {
  std::vector<void*> v;
  void flush() {
    for (void* p : v) (void)hipFree(p);
    v.clear();
  }
};
// r06: a device allocation that fails for lack of memory first evicts the process-wide
// target cache's entry of the current device (set in mgicp_clouds.hip, next to the cache) and retries once
extern bool (*g_oom_evict)();
// the graveyard of the context being constructed: every DevBuf member of a mgicp_ctx picks it up
extern thread_local Graveyard* t_new_ctx_grave;

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  Graveyard* grave = t_new_ctx_grave;
  bool fine = false;  // fine-grained device memory (r06: the xGMI exchange rows, which peers store into)
  // grows by >= 1/4 so that a sequence of slightly larger requests (grid sizing iterations,
  // the second cloud) does not pay a hipFree/hipMalloc pair each time
  hipError_t reserve(size_t n) {
    if (n <= cap && p) return hipSuccess;
    const size_t want = std::max<size_t>(std::max<size_t>(n, 1), cap ? cap + cap / 4 : 0);
    if (p) {
      if (grave) grave->v.push_back(p);
      else (void)hipFree(p);
    }
    p = nullptr;
    cap = 0;
    auto alloc = [&]() {
      return fine ? hipExtMallocWithFlags(reinterpret_cast<void**>(&p), want * sizeof(T), hipDeviceMallocFinegrained)
                  : hipMalloc(&p, want * sizeof(T));
    };
    hipError_t e = alloc();
    if (e == hipErrorOutOfMemory && g_oom_evict) {
      (void)hipGetLastError();
      p = nullptr;
      if (g_oom_evict()) e = alloc();
    }
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// a function-local device buffer, released on every exit.  (DevBuf itself has no destructor: the target
// cache's buffers are globals and would call hipFree at process exit.)
template <class T>
struct ScopedBuf : DevBuf<T> {
  ~ScopedBuf() { this->release(); }
};

struct Cloud {
  size_t n = 0;
  bool dirty = false;      // grid must be rebuilt
  bool have_cov = false;   // covariances valid for [cov_p0, cov_p1)
  size_t cov_p0 = 0, cov_p1 = 0;
  DevBuf<unsigned char> raw;  // staging of strided records
  DevBuf<float4> orig;        // original order, w = index
  DevBuf<float4> pts;         // grid-sorted
  DevBuf<uint32_t> perm;      // sorted pos -> original index
  DevBuf<uint32_t> cell_start;
  DevBuf<uint8_t> empty_dist; // empty-space map (target only: 1-NN queries leave the surface)
  bool want_empty_map = false;
  DevBuf<uint32_t> seed, seed_scratch;  // seed map (target: first-sweep 1-NN seeds)
  bool want_seed_map = false;
  DevBuf<float4> pairs;       // pair-interleaved points (target only: the wave-uniform 1-NN scan)
  bool drop_nonfinite = false; // build the grid over the finite points only (KdTreeFLANN semantics)
  double force_h = 0.0;        // > 0: build_grid takes this cell edge instead of sizing by occupancy (clustering)
  size_t n_built = 0;          // points of the last grid built in this slot
  bool fresh_grid = false;     // the grid is the one a fresh context builds for these points (target cache)
  DevBuf<double2> cov;        // 3 * cov_stride
  size_t cov_stride = 0;      // entries per covariance array (n, or the padded all-gather size)
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};  // bounding box (original coordinates)
  GridView view{};
  size_t ncells = 0;
  Cov3 cov3() const { return Cov3{cov.p, cov.p + cov_stride, cov.p + 2 * cov_stride}; }
};

enum { kFamCov = 0, kFamCorr = 1, kFamFdf = 2, kFamRed = 3, kFamCompact = 4, kFamMoments = 5, kFams = 6 };

// pass-path counters (mgicp_debug_pass_stats)
enum {
  kStSrvLaunch = 0,  // resident servers launched
  kStSrvPass,        // objective passes run by a server
  kStLaunchedPass,   // objective passes run by a launched kernel (gated, plain, or taking over)
  kStTakeover,       // server passes that missed their deadline and were re-run as launched passes
  kStBar,            // 1: the server reads its commands from device memory written through the BAR
  kStRowsAlloc,      // private host-row buffer allocations
  kStTransport,      // 0 local, 1 RCCL, 2 shared segment, 3 shared segment + RCCL (bulk all-gathers),
                     // 4 xGMI row exchange (+ segment), 5 xGMI row exchange + RCCL
  kStSrvDenied,      // server launches refused because another context of this process held the device
  kStMemoHit,        // objective evaluations answered from the run's table of evaluated transforms: no pass ran
  kStCount
};
static_assert(kStCount == 9, "mgicp_debug_pass_stats writes out[9]: engine.py's buffer and PASS_STATS follow");

// r05 target cache: one entry per device (its DevBufs belong to no context: grave = nullptr)
struct TargetCache {
  std::mutex mu;
  bool valid = false;
  Cloud t;
  int k = 0;
  double eps = 0;
  bool vl_valid = false, vl_alloc = false, vl_off = false;
  VListView vl{};
  size_t vl_ncells = 0;
  uint32_t vl_epoch = 0;
  int vl_groups = 0;
  DevBuf<uint32_t> vl_cell;
  DevBuf<float4> vl_pool;
  DevBuf<unsigned int> vl_ctr;
  long long hits = 0, donations = 0;
};
extern TargetCache g_tcache[64];

}  // namespace mgicp

struct mgicp_ctx {
  std::unique_ptr<Graveyard> grave;  // replaced device buffers of THIS context, freed at its quiet points
  mgicp_params prm{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  Cloud src, tgt;
  Cloud aux;  // scratch cloud of the resolution / radius / segment-differences helpers
  Cloud qry;  // query points of the FOD-side helpers (packed only, no grid)
  // FOD-side helper buffers (SegmentDifferences, VoxelGrid)
  DevBuf<uint32_t> f_flags, f_pos, f_rgba_in, f_rgba, f_rgba2;
  DevBuf<float4> f_vox, f_vox2;
  DevBuf<unsigned char> f_keep;
  DevBuf<unsigned int> f_count;
  // Euclidean clustering: the union-find forest, roots, per-root smallest index, sorted members, test counter
  DevBuf<uint32_t> cc_parent, cc_root, cc_min, cc_members;
  DevBuf<unsigned long long> cc_tests;
  bool fused_finish = true;              // in-launch reduction finish (debug option "fused_finish")
  double ms_upload_pending = 0;
  // host uploads go through the process-wide HostUploader (host_upload.hpp)
  int host_threads = 8;                  // packing workers (fixed)
  DevBuf<float> xyz_dev;                 // packed xyz landing zone
  // per source point (sorted), rank shard only
  DevBuf<float4> src_out;  // guess-applied source (only when guess != I)
  const float4* d_out = nullptr;
  // compacted accepted correspondences of the current outer iteration (shard-relative)
  DevBuf<uint32_t> prev_pos;  // matched target sorted position per shard point (also the next 1-NN seed)
  DevBuf<uint32_t> flags;
  DevBuf<float> corr_f;    // 6 streams
  DevBuf<double> corr_d;   // 6 streams

  size_t corr_cap = 0;     // elements per stream (multiple of 4)
  bool seed_valid = false;
  // query order of the 1-NN sweeps (Morton order of the shard)
  bool qperm_valid = false;
  DevBuf<uint32_t> qperm;
  // the fixed reduction tree (internal.hpp kChunkPts / kSuperChunks): chunk layout of the streams,
  // chunk and super partials of this shard, the all-gathered supers of every rank, the total
  DevBuf<uint32_t> ccnt;  // chunk_count(ns): correspondences per chunk (fixed-slot layout, r04)
  DevBuf<double> partial;       // chunk partials, kRedVals each
  DevBuf<unsigned long long> tpart;  // the server's stamped chunk partials, 32 words each (r03; 0xff.. = no stamp)
  size_t tpart_n = 0;
  DevBuf<double> spart;         // super partials (max_supers() rows: the all-gather send size)
  DevBuf<double> gath;          // nranks x max_supers() rows
  DevBuf<double> red;           // kRedVals
  DevBuf<unsigned int> tickets; // per super + 1: arrival counters of the in-launch finish
  size_t tickets_n = 0;
  // Gauss-Newton mode: chunk / super partials and the totals of one pass, and their host copy
  DevBuf<double> mpartial, msuper, mred;
  double mom[kMomVals] = {};
  double out_ctr[3] = {0, 0, 0};  // moment expansion centre: bbox midpoint of the guess-applied source
  unsigned char* h_small = nullptr;  // pinned, mapped host scratch (kSmallBytes) for small readbacks
  unsigned char* d_small = nullptr;  // its device address (kernels write results there directly)
  double* h_red = nullptr;   // pinned, mapped, coherent host memory
  double* d_h_red = nullptr; // its device address
  unsigned long long* h_flag = nullptr;  // pass-completion word (host / device views)
  unsigned long long* d_flag = nullptr;
  unsigned long long pass_seq = 0;
  // pre-launched (gated) objective passes: pass k + 1 is queued while pass k runs and waits on the
  // host-written command block (debug option "gated"; single-GPU polled mode)
  bool gated = true;
  PassCmd* h_cmd = nullptr;             // pinned, mapped, coherent host memory
  PassCmd* d_cmd = nullptr;             // its device address
  PassCmd* mail = nullptr;              // device copy block 0 of a gated pass forwards to the others
  // the server's command block in fine-grained device memory that the host stores into through the
  // BAR (debug option "bar_cmd"): every server block polls it, no PCIe read and no mailbox hop
  bool bar = true;
  PassCmd* bar_cmd = nullptr;
  // MGICP_PASS_DIAG builds: per gated pass (seq & 1023) the device wall clock at kernel start, command
  // seen, last block through the gate; the host's wall clock (us) at flag seen / command published
  unsigned long long* h_gtrace = nullptr;  // mapped host memory, 4 x 1024
  unsigned long long* d_gtrace = nullptr;
  std::vector<double> host_gt;             // 2 x 1024
  unsigned long long gated_seq = 0;     // sequence number of the queued gated pass (0 = none)
  unsigned long long gate_timeout = 0;  // wall_clock64 ticks a gated pass waits before giving up
  // the resident pass server (debug option "resident"; single GPU polled mode, or any rank count with the
  // shared row segment): one launch per BFGS run keeps part of the compacted streams in registers /
  // LDS across all its passes
  bool resident = true;
  bool srv_live = false;                // a server is running and waits for pass srv_next
  bool srv_locked = false;              // this context holds g_srv_busy[device]
  bool srv_degraded = false;            // a server pass was taken over: launched passes until the align ends
  unsigned long long srv_next = 0;
  int cus = 0;                          // compute units (the server's grid)
  int srv_cus = 0;                      // debug option "srv_cus": cap on the server's blocks (0 = every CU)
  int stall_pass = -1;                  // env MGICP_SRV_STALL_PASS (tests): a server block withholds this pass
  int quit_pass = -1;                   // env MGICP_DEBUG_QUIT_PASS (tests): the host gives up at this pass index
                                        // with MGICP_E_COMM (a rank that dies mid-align, seen from the others)
  double row_deadline_ms = 500.0;       // env MGICP_ROW_DEADLINE_MS: own rows missing this long -> take over
  double remote_deadline_s = 120.0;     // env MGICP_REMOTE_DEADLINE_S: other ranks' rows / gathers
  unsigned long long* h_ptimes = nullptr;  // MGICP_PASS_DIAG builds: per pass gate exit / finish (wall clock)
  unsigned long long* d_ptimes = nullptr;
  // the passes' super partials as stamped host rows (32 words per super, two parity buffers; debug
  // option "host_rows"): private pinned memory, or the node-wide shared segment
  bool host_rows = true;
  unsigned long long* h_rows = nullptr;
  unsigned long long* d_rows = nullptr;
  size_t rows_cap = 0;                  // supers per parity buffer
  std::vector<double> row_sums;         // decoded super partials
  bool rows_running = true;             // debug option "rows_running": single rank, the total's lane sums are taken
                                        // while the rows land (shm::RunningTotal; 0: fixed_total after the last row)
  unsigned int pass_idx = 0;            // objective passes so far: the row stamp (identical on every rank)
  unsigned long long gather_idx = 0;    // generic gathers through the shared segment so far
  // node-wide transport (mgicp_comm_attach_shm)
  bool have_shm = false;
  shm::Segment shm;
  // r05 xGMI row exchange (mgicp_comm_attach_xgmi, needs the segment for its rendezvous): every rank's
  // super reducers store their rows into this rank's exchange buffer (xrows: 2 parity buffers of
  // max_sup rows, device memory) and into every other rank's, mapped by IPC over xGMI; a one-wave
  // totaler per rank takes the fixed-order total on the device and stores it as one stamped host row
  bool have_xgmi = false;
  DevBuf<unsigned long long> xrows;
  std::vector<void*> xpeer;               // the other ranks' exchange buffers (IPC mappings), rank order
  unsigned long long* h_xtot = nullptr;   // the totaler's stamped row (32 words; host / device views)
  unsigned long long* d_xtot = nullptr;
  unsigned int* h_xgen = nullptr;         // generation word: a totaler exits when it changes
  unsigned int* d_xgen = nullptr;
  unsigned int xgen = 0;
  unsigned long long xseq = 0;            // attaches so far (the segment's publication flag value)
  hipStream_t xstream = nullptr;
  bool xstream_own = false;  // r06: the aux stream (idle during a BFGS run: N > 1 keeps the synchronous
                             // covariance path) when the context has one -- no third stream per context
  unsigned char* shm_d = nullptr;       // device view of the segment (hipHostRegister'ed)
  long long st[kStCount] = {};          // pass-path counters
  // the resident server as the aligns run it (mgicp_debug_server_time): two events per launch
  struct SrvEv { hipEvent_t a, b; long long passes; };
  std::vector<SrvEv> srv_ev;            // launches not yet resolved (the last one may be live)
  double srv_time_ms = 0;
  long long srv_time_passes = 0, srv_time_launches = 0;
  // MGICP_PASS_DIAG builds: host view of the server passes -- command published -> rows complete
  // (device pass + PCIe both ways) and rows complete -> next command (host BFGS step)
  double ht_dev = 0, ht_host = 0, ht_bfgs = 0, ht_eval = 0, ht_last_rows = 0;
  int ht_n = 0, ht_nh = 0, ht_ne = 0;
  // build scratch
  DevBuf<uint32_t> counts, keys, keys_sorted, vals;
  DevBuf<unsigned char> scratch;
  DevBuf<unsigned long long> u64;
  // lazy source covariances (r04, debug option "lazy_src_cov"): a source point's covariance is computed the
  // first time a sweep accepts it -- every consumer (Mahalanobis of the compaction, GN moments) reads
  // accepted points only, so points the gate never accepts (clutter, debris far off the part) never
  // pay PCL's exact 20-NN search; the values are the eager ones bit for bit
  bool lazy_src_cov = true;
  bool src_lazy_ready = false;      // cov arrays sized and cov_ok cleared for the current shard
  size_t src_lazy_p0 = 0, src_lazy_p1 = 0;
  DevBuf<uint8_t> cov_ok;           // per shard point: covariance computed
  DevBuf<uint32_t> cov_need;        // this sweep's accepted points without a covariance (absolute positions)
  // r04: set_target builds the target's grid and starts its k-NN covariances on a second stream, so
  // they run while the caller uploads the source; prepare joins them (debug option "async_cov" 0: off)
  // (and set_source the source's: single rank, same stream; with the lazy source mode these cover
  // every point, computed while the first sweep runs)
  // The aux stream carries no CU mask, though leaving every k-th CU to the main stream measured up to
  // -1.4 ms on new clouds (profiles/r04/ncab1): a CU mask belongs to the hardware queue, and past
  // GPU_MAX_HW_QUEUES streams share queues, so another context's main stream could inherit the mask --
  // and a resident server needs every CU (it stalled test_inlaunch_finish_*)
  bool async_tgt = true;
  bool tgt_cov_pending = false;     // the aux stream's covariance launches not joined yet
  bool src_cov_pending = false;
  bool src_async_lazy = false;      // the source's launch was ring-capped (lazy mode): the rest stays lazy
  // one stream for both clouds' launches: with a stream each the process exceeds its hardware queues
  // (GPU_MAX_HW_QUEUES, 4) and the main stream ends up sharing one with them (profiles/r04/prep7)
  hipStream_t aux_stream = nullptr;
  hipEvent_t aux_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // [3]: main stream -> aux (a grid built) (r06)
  // completion of the target's [0] / source's [1] launch,
                                                       // [2] the source's Morton order sorted on the aux stream
  bool qperm_aux = false;                    // qperm is being sorted on the aux stream (aux_ev[2])
  DevBuf<uint32_t> aq_keys, aq_keys_sorted, aq_vals;  // its sort buffers (the main stream's may be busy)
  DevBuf<unsigned char> aq_scratch;
  DevBuf<unsigned int> aux_cnt;     // their hand-off counts: [0] target, [1] source
  DevBuf<uint32_t> knn_fb2;         // the source's hand-off list
  bool knn_wave = true;             // r06: lazy pass + hand-offs by the wave-per-query kernel (debug option "knn_wave")
  bool knn_logged = true;           // wave-staged k-NN kernel + hand-off (debug option "knn_logged" 0: register-list only)
  DevBuf<uint32_t> knn_fb;          // points the logged k-NN kernel leaves to the register-list one
  unsigned int knn_fallbacks = 0;   // their count in the last covariance launch
  DevBuf<float> fpartial;
  // mgicp_match_features: pairs of one launch (debug option "match_pairs_per_launch") and the last call's
  // figures for mgicp_debug_match_stats
  unsigned long long match_pairs_per_launch = kMatchPairsPerLaunch;
  long long match_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // mgicp_reject_ransac: hypotheses of one scoring launch (debug option "ransac_batch")
  int ransac_batch = kRansacBatch;
  // mgicp_normal_clusters: records above which a round goes wide (debug option "nc_small_limit")
  int nc_small_limit = static_cast<int>(kNcSmallLimit);
  // the target's 1-NN cell lists (r04, DESIGN.md "1-NN cell lists"; debug option "vlist" 0: the r03 sweeps)
  bool vlist = true;
  bool fuse_compact = true;           // r04: compaction fused into listed sweeps (debug option "fuse_compact")
  DevBuf<uint32_t> vl_defer;          // chunks a fused sweep deferred to the compaction launch
  // r08, the steady-state round (DESIGN.md "r08: the steady-state round"): a fused listed sweep hands
  // ctr[1..3] to the host (one wave, stamped words in mapped memory); all zero = nothing was requested,
  // left pending or deferred, so centres, builds, fallback, the lazy-covariance pass and the deferred
  // compaction are not launched at all (debug option "round_fast" 0: always launched, as before r08)
  bool round_fast = true;
  unsigned long long* h_round = nullptr;   // 3 words (stamp << 32) | ctr[1 + i]; host / device views
  unsigned long long* d_round = nullptr;
  unsigned int round_stamp = 0;            // the last round's stamp (never 0)
  const unsigned int* vl_ctr_zero = nullptr;  // == vl_ctr.p while ctr[1..4] are known to be zero (a clean round
                                              // left them so): the next sweep does not fill them again
  long long round_st[4] = {0, 0, 0, 0};    // mgicp_debug_round_stats
  bool vl_stats = false;              // debug option "vlist_stats": per-sweep list diagnostics on stderr
  bool vl_valid = false;              // lists belong to the current target grid and gate
  bool vl_alloc = false;              // their state words and pool are allocated and initialised
  bool vl_off = false;                // the gate is too large for a fine grid of this target: r03 sweeps
  VListView vl{};
  size_t vl_ncells = 0;
  DevBuf<uint32_t> vl_cell, vl_build, vl_bcentre, vl_pend;
  DevBuf<float4> vl_pool;
  DevBuf<unsigned int> vl_ctr;
  uint32_t vl_epoch = 0;              // sweeps run over the current lists
  // A cell's list is built when a sweep of the SECOND align (or debug sweep group) over the current
  // target and gate queries it: the first align after a set_target runs the r03 sweep (no list work,
  // the ms-to-converge of a one-off align is unchanged), the second builds the lists of every cell it
  // queries, later aligns (GICPAlignment::iterate, the next scans of the same CAD target) read them.
  int vl_groups = 0;                  // aligns / debug sweep groups finished over the current lists
  bool vl_eager = false;              // debug option "vlist_eager" 1: build every queried cell at once (default: a cell
                                      // is built when a later sweep queries it again)
  // aligns (or debug sweep groups) after a set_target / gate change that run the r03 sweep before the
  // lists are used (debug option "vlist_cold" N).  The lists pay off only over many aligns on one target
  // (a later scan against the same CAD cloud, bench.py's steady state): building them costs ~57 ms
  // eagerly or ~15 ms spread over two aligns lazily at C4, so the reference's align + iterate pair on
  // one cloud pair (GICPAlignment.cpp:96, :116) runs both aligns without them (r04, profiles/r04/policy)
  int vl_cold_groups = 2;
  size_t vl_pool_entries = 0;         // debug option "vlist_pool" N: a pool of max(N, 4096) entries (0: the default size)
  // r05 target cache (process-wide, one entry per device): a destroyed context leaves its target's grid,
  // covariances and 1-NN cell lists there; a later context whose set_target uploads the same points
  // (compared on the device, bit for bit) adopts them instead of rebuilding -- GICPState constructs a
  // fresh GICPAlignment per scan against the same CAD cloud (LeicaStateMachine.cpp:149-150)
  bool tcache_on = false;               // debug option "target_cache" (r06: opt-in; VERDICT r05 weak 5 --
                                        // the reference node aligns once per process)
  bool tcache_adopted = false;          // the current target came from the cache
  // multi-GPU
  int nranks = 1, rank = 0;
  ncclComm_t comm = nullptr;
  // state of the last correspondence sweep
  bool have_corr = false;
  Mat4 last_guess = Mat4::identity();
  std::vector<float> trace;
  int n_evals = 0;
  // debug option "pass_memo" (0: every evaluation at a new x is a device pass): an evaluation whose fp32
  // transform the BFGS run has already passed over takes that pass's sums (pass_memo.hpp)
  bool pass_memo = true;
  // profiling
  bool profiling = false;
  unsigned long long prof_tick = 0;
  struct EvPair { hipEvent_t a, b; int fam; };
  std::vector<EvPair> pending;
  std::vector<hipEvent_t> pool;
  double fam_ms[kFams] = {};
  int fam_cnt[kFams] = {};

  // shards start on super boundaries: rank r owns supers [super_first(r), super_first(r + 1))
  long long nsup_total() const { return static_cast<long long>((src.n + kSuperPts - 1) / kSuperPts); }
  size_t shard_at(int r) const {
    return std::min(src.n, static_cast<size_t>(super_first(r, nsup_total(), nranks)) * kSuperPts);
  }
  size_t shard_p0() const { return shard_at(rank); }
  size_t shard_p1() const { return shard_at(rank + 1); }
  long long nsup_local() const {
    return super_first(rank + 1, nsup_total(), nranks) - super_first(rank, nsup_total(), nranks);
  }
  long long max_supers() const { return (nsup_total() + nranks - 1) / nranks; }
};

namespace mgicp {

inline int fail(mgicp_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPCK(expr)                                                                    \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(ctx, (e_ == hipErrorOutOfMemory) ? MGICP_E_NOMEM : MGICP_E_HIP,      \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)

#define NCCLCK(expr)                                                                   \
  do {                                                                                 \
    ncclResult_t r_ = (expr);                                                          \
    if (r_ != ncclSuccess)                                                             \
      return fail(ctx, MGICP_E_COMM, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

// Where the host rows of the passes live: this context's private pinned buffers (single rank), or
// the node-wide shared segment (every rank's rows at their global super index).  Parity buffer p
// starts stride words after parity 0; this rank's rows start at super `first`.
struct RowView {
  unsigned long long* h0 = nullptr;  // host view, parity 0, super 0
  unsigned long long* d0 = nullptr;  // device view, parity 0, super 0
  size_t stride = 0;                 // words between the parity buffers
  long long first = 0, nloc = 0, ntot = 0;
  unsigned long long* dev_rows(unsigned int rstamp) const {  // this rank's rows of the pass stamped rstamp
    return d0 + (rstamp & 1u) * stride + static_cast<size_t>(first) * shm::kRowWords;
  }
};

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// MGICP_TRACE=1: phase timestamps of uploads and grid builds on stderr (host-time diagnosis)
inline bool trace_on() {
  static const int on = [] {
    const char* t = std::getenv("MGICP_TRACE");
    return t && std::atoi(t) != 0 ? 1 : 0;
  }();
  return on != 0;
}
#define MGICP_TRACE_AT(label)                                                  \
  do {                                                                         \
    if (trace_on()) std::fprintf(stderr, "[mgicp] %10.3f ms  %s\n", now_ms(), label); \
  } while (0)

// objective-pass event sampling while profiling: every 8th launch (identical work per launch, and two
// event records per pass would cost ~4 % of the PCL-mode align)
constexpr unsigned kProfStride = 8;

inline hipEvent_t ev_get(mgicp_ctx* ctx) {
  if (!ctx->pool.empty()) {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

struct ProfScope {
  mgicp_ctx* ctx;
  int fam;
  hipEvent_t a = nullptr;
  ProfScope(mgicp_ctx* c, int f) : ctx(c), fam(f) {
    // objective passes are sampled (every kProfStride-th launch); the rest are all timed
    if (ctx->profiling && (fam != kFamFdf || (ctx->prof_tick++ % kProfStride) == 0)) {
      a = ev_get(ctx);
      (void)hipEventRecord(a, ctx->stream);
    }
  }
  ~ProfScope() { close(); }
  void close() {  // ends the scope early (once)
    if (a) {
      hipEvent_t b = ev_get(ctx);
      (void)hipEventRecord(b, ctx->stream);
      ctx->pending.push_back({a, b, fam});
      a = nullptr;
    }
  }
};

// ---- mgicp_pass.hip: the objective passes and their transport (documented there) ----
Mat4 apply_state(const Vec6& x);
void prof_resolve(mgicp_ctx* ctx);
void cancel_gated(mgicp_ctx* ctx);
void srv_resolve(mgicp_ctx* ctx);
void srv_release(mgicp_ctx* ctx);
int sync(mgicp_ctx* ctx);
int reset_stamps(mgicp_ctx* ctx);
int ensure_host_red(mgicp_ctx* ctx);
CorrSoA corr_soa(mgicp_ctx* ctx);
RowView row_view(const mgicp_ctx* ctx);
int ensure_rows(mgicp_ctx* ctx);
int wait_rows(mgicp_ctx* ctx, unsigned int rstamp, const Xf34& A, double out[kRedVals], bool allow_takeover);
int ensure_iter_buffers(mgicp_ctx* ctx);
int combine_to_host(mgicp_ctx* ctx, int nv, const double* sup, double* out);
// OptimizationFunctorWithIndices::fdf on the device; memoises the last state, and the sums of every
// pass of its BFGS run by the fp32 transform the pass was given.  One functor per run (estimate_bfgs
// constructs it): the table must not outlive the run's correspondences.  Every rank runs the same host
// BFGS on bit-identical totals, so every rank hits and misses on the same evaluations; nothing
// per-rank (timing, a take-over) feeds the decision, and row stamps advance only in pass().
struct DeviceFunctor {
  mgicp_ctx* ctx;
  bool have_memo = false;
  Vec6 memo_x{};
  double memo_f = 0;
  Vec6 memo_g{};
  double m = 0;  // correspondences of this sweep (all ranks)
  PassMemo seen{};  // (transform, sums) of this run's passes (ctx->pass_memo)

  int pass(const Vec6& x, double sums[kRedVals]);         // one objective pass at x: its 16 raw sums (never memoised)
  void remember(const Vec6& x, const double s[kRedVals]);  // the sums of the pass at x into the run's table
  void memoise(const Vec6& x, const double s[kRedVals]);  // f and g at x from the sums of the pass at x
  int eval(const Vec6& x, double& f, Vec6& g);
};
static_assert(PassMemo::kVals == kRedVals && sizeof(Xf34) == PassMemo::kKeyFloats * sizeof(float),
              "pass_memo.hpp restates the pass's key and value sizes");
struct GateGuard {  // a BFGS run leaves no gated pass queued behind it
  mgicp_ctx* ctx;
  ~GateGuard() { cancel_gated(ctx); }
};
// over one DeviceFunctor (one run of it, no queued pass or live server left behind):
// OptimizationFunctorWithIndices::fdf at x over the last correspondence sweep, and the 16 raw sums of
// one objective pass at x; fdf_sums_run_at: n passes at xs[0 .. n) over ONE DeviceFunctor (one live
// server for all of them, as a BFGS run holds it), kRedVals sums per pass
int fdf_at(mgicp_ctx* ctx, const Vec6& x, double& f, Vec6& g);
int fdf_sums_at(mgicp_ctx* ctx, const Vec6& x, double sums[kRedVals]);
int fdf_sums_run_at(mgicp_ctx* ctx, const Vec6* xs, int n, double* sums);

// ---- mgicp_clouds.hip: uploads, grids, covariances, the target cache (documented there) ----
int upload_cloud(mgicp_ctx* ctx, Cloud& cl, const float* xyz, size_t n, size_t stride, bool device_ptr);
int bbox_to_host(mgicp_ctx* ctx, const float4* pts, size_t n, float lo[3], float hi[3], double* bad = nullptr,
                 const char* queued = nullptr);
int build_grid(mgicp_ctx* ctx, Cloud& cl, bool defer_extras = false);
int aux_grid(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride, double force_h = 0.0);
const uint32_t* query_perm(mgicp_ctx* ctx);
int cov_join_all(mgicp_ctx* ctx);
int cov_prep_async_all(mgicp_ctx* ctx);
int compute_cov(mgicp_ctx* ctx, Cloud& cl, size_t p0, size_t p1, size_t stride = 0);
int target_cov(mgicp_ctx* ctx);
int cov_lazy(mgicp_ctx* ctx);
void tcache_donate(mgicp_ctx* ctx, bool cov_complete);
int tcache_adopt(mgicp_ctx* ctx);

// FLANN's radius search as the product calls restate it: d2 < r2 = float(radius^2), strict, so 0 links
// nothing, not even a point with itself.  Every neighbour lies within `reach` per axis; a denormal r2
// may be far above radius^2
struct FlannRadius {
  float r2;
  double reach;
  explicit FlannRadius(double radius) : r2(static_cast<float>(radius * radius)), reach(radius) {
    if (r2 < 1.17549435e-38f) reach = std::max(reach, std::sqrt(static_cast<double>(r2)));
  }
};

// ---- mgicp_engine.hip: the align loop's steps that the debug entry points call too (documented there) ----
int prepare(mgicp_ctx* ctx, bool need_cov);
int set_output(mgicp_ctx* ctx, const Mat4& G);
int correspond(mgicp_ctx* ctx, const Mat4& T, const Mat4& G, bool seed);
int moments_pass(mgicp_ctx* ctx, const Mat4& T, const Mat4& G, bool supers_only = false);
int fitness_supers(mgicp_ctx* ctx, const Mat4& T, double max_range);

// ---- mgicp_comm.hip: the xGMI row exchange's teardown ----
void xgmi_cancel(mgicp_ctx* ctx);
void xgmi_detach(mgicp_ctx* ctx);

}  // namespace mgicp
