// mgicp_internal.hpp -- shared device-side layouts and kernel launchers of libmgicp.so.
//
// HBM layout (DESIGN.md "Data layout"): every cloud lives in a uniform grid sorted by
// linear cell index (z-major, then y, then x; stable in the original point index), so a
// row of cells is one contiguous range of the point array:
//   pts        float4[n]      (x, y, z, bit_cast<float>(original index))
//   cell_start uint32[nc + 1] exclusive prefix of per-cell counts (dense over the bbox)
//   cov        3 x double2[n] symmetric covariance {c00,c01},{c02,c11},{c12,c22}
// Per source point of the shard (sorted order), rewritten every outer iteration:
//   nn_pos     uint32[n]      matched target sorted position (UINT32_MAX = rejected)
//   flags/pos  uint32[n+1]    acceptance and its exclusive scan (compacted slot)
// Accepted correspondences: CorrSoA (below), 72 bytes each.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mgicp {

struct GridView {
  float ox, oy, oz;   // grid origin (bbox min)
  float h, inv_h;     // cell edge and its reciprocal
  float slop;         // absolute rounding slack for ring lower bounds (metres)
  int nx, ny, nz;
  const uint32_t* cell_start;  // nx*ny*nz + 1
  const float4* pts;           // sorted points
  // optional empty-space map: per cell, the Chebyshev distance (in cells) to the nearest
  // non-empty cell, capped at kEmptyCap + 1; rings closer than it hold no point
  const uint8_t* empty_dist;
  // optional seed map (with empty_dist): per cell within the cap, the sorted position of a point in
  // a Chebyshev-nearest non-empty cell -- a real candidate that seeds an unseeded 1-NN search
  const uint32_t* seed;
  // optional pair-interleaved copy of pts for the wave-uniform 1-NN scan (2 float4 per pair of
  // points: x0 x1 y0 y1 | z0 z1 w0 w1; pair_count(n) pairs, far sentinels past n)
  const float4* pairs;
};

#ifndef MGICP_EMPTY_CAP
#define MGICP_EMPTY_CAP 15
#endif
constexpr int kEmptyCap = MGICP_EMPTY_CAP;

struct Cov3 {  // SoA triple of double2 arrays
  double2* a;  // {m00, m01}
  double2* b;  // {m02, m11}
  double2* c;  // {m12, m22}
};

// Accepted correspondences of one outer iteration, compacted in grid-sorted source order and
// stored as 12 streams (each padded to a multiple of 4 elements) so that an objective pass reads
// 72 bytes per correspondence with 16-byte loads and no branch.
struct CorrSoA {
  float *sx, *sy, *sz, *qx, *qy, *qz;
  double *m00, *m01, *m02, *m11, *m12, *m22;
};

// Number of values reduced per objective pass:
//   [0] f-sum  [1..3] g_t sum  [4..12] Rsum (row-major)  [13] count  [14..15] pad
constexpr int kRedVals = 16;
constexpr int kMaxK = 32;  // largest k_correspondences_ the covariance kernel serves
constexpr int kRedThreads = 256;
// Number of values reduced per Gauss-Newton moment pass (MGICP_SOLVER_GN):
//   [0] sum r0'M r0  [1..12] sum (M r0) w'  [13..72] sum M_p (w w')_q  [73] count  [74..79] pad
constexpr int kMomVals = 80;

// The fixed global reduction tree of every sharded sum (objective passes, Gauss-Newton moments,
// fitness): chunks of kChunkPts grid-sorted source positions (one wave each), supers of
// kSuperChunks chunks, then the total over supers.  Shards start on super boundaries (rank r owns
// supers [nsup * r / N, nsup * (r + 1) / N)), so every N reproduces the N = 1 sums bit for bit.
constexpr int kChunkPts = 1024;
constexpr int kSuperChunks = 32;
constexpr size_t kSuperPts = static_cast<size_t>(kChunkPts) * kSuperChunks;
inline int chunk_count(size_t n) { return static_cast<int>((n + kChunkPts - 1) / kChunkPts); }
__host__ __device__ inline long long super_first(int r, long long nsup, int nranks) {
  return nsup * r / nranks;
}
__host__ __device__ inline int super_owner(long long s, long long nsup, int nranks) {
  int r = static_cast<int>(s * nranks / (nsup > 0 ? nsup : 1));
  if (r > nranks - 1) r = nranks - 1;
  while (r > 0 && s < super_first(r, nsup, nranks)) --r;
  while (r < nranks - 1 && s >= super_first(r + 1, nsup, nranks)) ++r;
  return r;
}

// Xform as 3x4 row-major float (the top three rows of an Eigen::Matrix4f).
struct Xf34 { float m[12]; };

// Command block of a pre-launched (gated) objective pass, in pinned mapped host memory (and its
// device-memory forward).  Self-validating without fences: every 8-byte half carries one payload
// word (low 32 bits) and the low 32 bits of the pass's sequence number (high 32 bits); aligned
// 8-byte stores and loads are single-copy atomic on both sides, so a reader that finds the stamp
// in all kCmdWords halves holds a complete command of that pass -- in the same PCIe round trip
// that detects it.  Words: [0..11] A (Xf34 bit patterns), [12] op, [13] sweep direction, [14] the
// pass's row stamp (host-row passes: the objective-pass index, identical on every rank, that stamps
// the super rows and selects their parity buffer).  A waiting block that finds a complete command
// with a LATER sequence number was left behind by a cancel and exits.
constexpr unsigned int kPassRun = 1;
constexpr unsigned int kPassCancel = 2;
constexpr int kCmdWords = 15;
struct alignas(128) PassCmd {
  unsigned long long h[16];
};
struct Rot33d { double m[9]; };

// ---- launchers (mgicp_kernels.hip); all asynchronous on `s` ----
hipError_t launch_pack_points(const void* raw, size_t n, size_t stride, float4* out,
                              hipStream_t s);
hipError_t launch_bbox(const float4* pts, size_t n, float* partial /*nb*8*/, int nb,
                       hipStream_t s);
// linear cell index (z-major) of every point: the keys of the grid's sort
hipError_t launch_cell_keys(const float4* pts, size_t n, float ox, float oy, float oz,
                            float inv_h, int nx, int ny, int nz, uint32_t* keys, hipStream_t s);
// r06: the grid's sizing sketch (cell_sketch_kernel): kSketchR one-byte HyperLogLog registers of the
// occupied cells at each of kSketchScales cell sizes (1 / inv[k]) over origin (ox, oy, oz), in one pass;
// `partial` holds (kSketchBlocks + 32) * kSketchScales * kSketchR bytes, the merged registers land in `out`
constexpr int kSketchScales = 16;
constexpr int kSketchLog2R = 7;  // 128 registers per size (~9 % error): 8 KiB of LDS, so a sketch block
                                  // fits beside the source's k-NN (12 KiB per wave, 12 waves per CU)
constexpr int kSketchR = 1 << kSketchLog2R;
constexpr int kSketchBlocks = 1024;  // of 256 threads (4 per CU: the per-scale LDS read-check is latency-bound)
struct SketchScales { float inv[kSketchScales]; };
hipError_t launch_cell_sketch(const float4* pts, size_t n, float ox, float oy, float oz, const SketchScales& sc,
                              uint8_t* partial, uint8_t* out, hipStream_t s);
// r06: cell_start[0..nc] of a grid from its sorted keys (no histogram): `ends` (nc + 1 words) is
// zeroed and receives each non-empty cell's end, then an exclusive max-scan gives the starts
size_t cell_start_scratch_bytes(size_t nc);
hipError_t launch_cell_starts(const uint32_t* keys_sorted, size_t n, size_t nc, uint32_t* ends, uint32_t* cell_start,
                              void* scratch, size_t scratch_bytes, hipStream_t s);
hipError_t launch_gather_sorted(const float4* pts, const uint32_t* perm, size_t n,
                                float4* out, hipStream_t s);
hipError_t launch_xform_points(const float4* in, size_t n, Xf34 T, float4* out,
                               hipStream_t s);
// k-NN covariances of [p0, p1).  fb / fb_count (nullable): the logged-threshold kernel, which lists
// in fb (count in *fb_count, device, zeroed by the caller) the points it leaves to the register-list
// kernel; run that list with perm = fb, p0 = 0, p1 = count, fb = nullptr.
// ring_cap >= 0 (logged kernel only): a query whose search passes that ring gives up -- no
// covariance, not listed in fb, ok[p] stays 0; every other query sets ok[p] = 1 (ok nullable)
// r06: exact k-NN covariances with one wave per query (the lazy pass, the hand-off), queries list[i] for
// i < *count (count non-null, device-side) or n; blocks <= 0: one wave per query
hipError_t launch_knn_wave(const GridView& g, int k, double eps, const uint32_t* list, const unsigned int* count,
                           size_t n, Cov3 cov, hipStream_t s, int blocks = 0);
hipError_t launch_knn_cov(const GridView& g, int k, double eps, size_t p0, size_t p1,
                          Cov3 cov, const uint32_t* perm /*nullable: query order*/, uint32_t* fb,
                          unsigned int* fb_count, hipStream_t s, int ring_cap = -1, uint8_t* ok = nullptr,
                          int chain = 0 /*> 0: the hand-off launch follows on s, that many blocks, device count*/,
                          bool wave_handoff = true /*r06: the chained hand-off by knn_wave_kernel*/);
// nn_pos: per source point (shard-relative) the matched target sorted position, UINT32_MAX when
// rejected; with `seeded` its previous contents seed the exact 1-NN search.  flags: 1 if accepted.
// The wave-uniform 1-NN sweep (needs tgt.pairs); lanes the union scan does not settle finish with the
// per-lane search (limits: mgicp_kernels.hip, launch_correspond_wave)
hipError_t launch_correspond_wave(const GridView& tgt, const float4* src, size_t p0, size_t p1, Xf34 T,
                                  double thr, int seeded, uint32_t* nn_pos, uint32_t* flags,
                                  const uint32_t* qperm /*nullable: query order*/, hipStream_t s);

// ---- the target's 1-NN cell lists (r04; DESIGN.md "1-NN cell lists") ----
// A fine uniform grid over the target's bbox grown by the gate.  Per cell: the target points that can
// be the exact 1-NN (fp32 FLANN d2, original-index tie-break) of some query in the cell whose d2 is
// below the gate -- a superset, pruned by the affine dominance test against 9 anchor points -- or
// "reject" (no target point within the gate of the cell).  Lists are built the first time a sweep
// queries the cell and persist until the target or the gate changes.
constexpr uint32_t kVlNotBuilt = 0xFFFFFFFFu;  // never queried
constexpr uint32_t kVlRequested = 0xFFFFFFFEu; // queued for this sweep's build
constexpr uint32_t kVlOverflow = 0xFFFFFFFDu;  // more than kVlMaxList entries / candidates / pool full
constexpr uint32_t kVlReject = 0xFFFFFFFCu;    // no target point within the gate of the cell
constexpr uint32_t kVlTouched = 0x80000000u;   // | epoch: first queried in sweep `epoch` (built when queried
                                               // again in a later sweep); values below: (off4 << 6) | count
constexpr int kVlLong = 63;                    // count field 63: a long list -- its true count in the x bits of a
                                               // header entry at off, its entries from off + 4
                                               // (lists padded to a multiple of 4 with far sentinels; off4 = list
                                               // start / 4, < 2^25)
struct VListView {
  float ox, oy, oz;      // fine grid origin
  float c, inv_c;        // fine cell edge and its float reciprocal
  float es;              // box growth covering the fp32 cell assignment of queries
  int nx, ny, nz;
  double gate;           // max correspondence distance the lists are built for
  uint32_t* cell;        // nx * ny * nz states / (off << 6 | count)
  float4* pool;          // list entries {x, y, z, bits(sorted target position)}
  const float4* tpts;    // the target's sorted points (w = original index: exact-distance ties only)
  uint32_t pool_cap;     // entries (< 2^26)
  unsigned int* ctr;     // [0] pool head (persistent), [1] cells requested, [2] queries pending, [3] deferred
                         // chunks, [4] cells left to the build's second pass (per sweep)
  uint32_t* build;       // requested cells of this sweep
  uint32_t* bcentre;     // per requested cell: sorted position of the cell centre's 1-NN (or none)
  uint32_t build_cap;
  uint32_t* pend;        // shard-relative positions of this sweep's queries without a list
  uint32_t epoch;        // this sweep's number (1 .. 2^30 - 1)
  int eager;             // 1: build a cell's list at its first query (else at its first query in a later sweep)
};
// one sweep over the lists: listed queries answered at once, reject cells rejected, the others
// queued (pend) and their cells requested; then the requested cells' lists are built and the
// pending queries answered by the exact per-lane search (seeded like correspond_wave_kernel's)
// the compaction fused into a listed sweep (vl_query_compact_kernel): its inputs; chunks it cannot
// finish (a pending query, a lazy source covariance not computed yet) are listed in `defer`, count
// in VListView::ctr[3], for launch_compact(..., defer, ctr + 3)
struct FusedCompact {
  Cov3 cov_s, cov_t;
  Rot33d R;
  const uint8_t* cov_ok;  // lazy source mode: per shard point, covariance computed (nullptr: all are)
  uint32_t* ccnt;
  uint32_t* defer;
  CorrSoA out;
};
hipError_t launch_vl_sweep(const GridView& tgt, const VListView& vl, const float4* src, size_t p0, size_t p1,
                           Xf34 T, double thr, int seeded, uint32_t* nn_pos, uint32_t* flags, int cus,
                           hipStream_t s, const FusedCompact* fc = nullptr);
// r08, the sweep in its two halves (launch_vl_sweep = both, counters zeroed, no verdict).
// launch_vl_queries: the query kernel alone; zero_ctr false when ctr[1..4] are known to be zero (the
// round before was clean); verdict (mapped host memory, 3 words) non-null: one wave then stores
// (stamp << 32) | ctr[1 + i] into verdict[i].  launch_vl_follow: centres, the two builds, the fallback --
// every one of them a no-op when ctr[1] == ctr[2] == 0.
hipError_t launch_vl_queries(const VListView& vl, const float4* src, size_t p0, size_t p1, Xf34 T, double thr,
                             uint32_t* nn_pos, uint32_t* flags, hipStream_t s, const FusedCompact* fc, bool zero_ctr,
                             unsigned long long* verdict, unsigned int stamp);
hipError_t launch_vl_follow(const GridView& tgt, const VListView& vl, const float4* src, size_t p0, size_t p1,
                            Xf34 T, double thr, int seeded, uint32_t* nn_pos, uint32_t* flags, int cus,
                            hipStream_t s);
// lazy source covariances (r04): shard positions k with flags[k] && !cov_ok[k] -> list (absolute
// positions p0 + k, *count of them), cov_ok[k] = 1
hipError_t launch_cov_need(const uint32_t* flags, uint8_t* cov_ok, size_t p0, size_t n, uint32_t* list,
                           unsigned int* count, hipStream_t s);
// diagnostics (mgicp_debug_option "vlist_stats"): per built cell list lengths histogram etc. into out[64]
hipError_t launch_vl_stats(const VListView& vl, size_t ncells, unsigned long long* out /*device, 64*/, hipStream_t s);
size_t     pair_count(size_t n);
hipError_t launch_pairs(const float4* pts, size_t n, float4* out, hipStream_t s);
// Morton keys (30 bit, bbox lo, 1024 / extent = inv) of points [p0, p0 + n) and values 0..n-1
hipError_t launch_morton_keys(const float4* pts, size_t p0, size_t n, const float lo[3], float inv,
                              uint32_t* keys, uint32_t* vals, hipStream_t s);
// accepted correspondences -> their chunk's run of the streams (fixed slots: chunk c at c *
// kChunkPts, ccnt[c] of them, pads to a multiple of 4 zeroed), computing the Mahalanobis matrices
// on the way
// defer (nullable): only the chunks a fused listed sweep deferred (list + device count)
hipError_t launch_compact(const float4* src, const float4* tpts, const Cov3& cov_s,
                          const Cov3& cov_t, Rot33d R, const uint32_t* nn_pos,
                          const uint32_t* flags, size_t p0, size_t p1, uint32_t* ccnt, CorrSoA out, hipStream_t s,
                          const uint32_t* defer = nullptr, const unsigned int* defer_count = nullptr, int cus = 0);
// objective pass over the shard's chunks (ns source positions): chunk partials (partial,
// chunk_count(ns) x kRedVals), super partials (spart), and with `out` the total (in-launch).
// tickets: one per super + one, zero between passes.  done_flag (nullable, mapped host memory):
// the finishing wave stores `seq` there with a system-scope release after `out`, so the host can
// poll instead of synchronising the stream
// host_rows (nullable): super partials as stamped host rows (stamp rstamp, this pass's parity buffer
// at the rank's first super; tickets counted modulo the supers' sizes) instead of spart / out
hipError_t launch_fdf_soa(const CorrSoA& c, const uint32_t* ccnt, size_t ns, Xf34 A,
                          double* partial, double* spart, int nb, unsigned int* tickets, double* out, int reverse,
                          unsigned long long* done_flag, unsigned long long seq, hipStream_t s,
                          unsigned long long* host_rows = nullptr, unsigned int rstamp = 0);
// the same pass pre-launched before its state is known: block 0 waits for cmd->seq == seq (or for
// `timeout_ticks` of wall_clock64) and forwards the command to `mail` (device memory) for the other
// blocks; then every block runs with its A / reverse, or exits on a cancel
hipError_t launch_fdf_soa_gated(const CorrSoA& c, const uint32_t* ccnt, size_t ns,
                                double* partial, double* spart, int nb, unsigned int* tickets, double* out,
                                unsigned long long* done_flag, unsigned long long seq, const PassCmd* cmd,
                                PassCmd* mail, unsigned long long timeout_ticks,
                                unsigned long long* gtrace /*nullable: diagnostics*/,
                                int host_pollers /*blocks [0, host_pollers) poll the host copy*/, hipStream_t s);
int        fdf_grid_blocks(size_t ns, int max_blocks = 2048);
// the resident pass server (one launch per BFGS run, see mgicp_kernels.hip): passes seq0, seq0 + 1,
// ... each run on the command with that stamp, until a cancel (or a later command); bench_passes > 0
// (timing): that many passes of A back to back without commands.  fdf_server_blocks: its grid for a
// shard of ns positions on `cus` CUs (0: not servable, use the launched passes)
int        fdf_server_blocks(size_t ns, int cus);
// r05, N > 1 over xGMI: the other ranks' exchange buffers (IPC-mapped device memory), at this rank's
// first super; a super's reducer stores its row into its own buffer (host_rows) and into every one of
// these, so each rank's buffer receives every rank's rows
constexpr int kMaxPeers = 8;
struct PeerRows {
  unsigned long long* p[kMaxPeers];
  int n;
};
hipError_t launch_fdf_server(const CorrSoA& c, const uint32_t* ccnt, size_t ns, double* partial,
                             double* spart, unsigned int* tickets, double* out, unsigned long long* done_flag,
                             unsigned long long seq0, const PassCmd* cmd, PassCmd* mail,
                             unsigned long long timeout_ticks, unsigned long long* ptimes /*nullable*/,
                             int bench_passes, Xf34 A,
                             unsigned long long* host_rows /*nullable: super rows to the host, parity 0*/,
                             size_t rows_stride /*words from the parity-0 to the parity-1 row buffer*/, int nb,
                             int pollers /*blocks reading cmd themselves (1 or nb)*/,
                             int stall_pass /*tests: -1, or the pass the last block withholds*/,
                             unsigned long long* tpart /*nullable: stamped chunk partials, 32 words per chunk (r03)*/,
                             hipStream_t s, const PeerRows* peers = nullptr);
// r05 xGMI totaler (one wave, persistent for a BFGS run): for passes stamp0, stamp0 + 1, ... waits until
// all nsup rows of the pass in this rank's exchange buffer (rows0, parity buffers `stride` words apart)
// carry the pass's stamp, takes the fixed-order total (shm::fixed_total's tree) and stores it as one
// stamped 32-word row at `out` (mapped host memory); exits when *gen_word != gen or after
// `timeout_ticks` without a complete pass
hipError_t launch_xgmi_total(const unsigned long long* rows0, size_t stride, long long nsup, unsigned int stamp0,
                             unsigned long long* out, const unsigned int* gen_word, unsigned int gen,
                             unsigned long long timeout_ticks, hipStream_t s);

// super partials of nch chunk partials of nv (kRedVals or kMomVals) values
hipError_t launch_super_reduce(const double* chunk, int nch, int nv, double* sup, hipStream_t s);
// totals of nsup supers held as nranks rows of maxsup (row r: rank r's supers, from super_first(r))
// tests: wave_sum x 16 vs wave_sum16 on in[w][lane][16] (mgicp_debug_wave_reduce)
hipError_t launch_wave_reduce_check(const double* in, int nwaves, double* out_tree, double* out_rs, hipStream_t s);
hipError_t launch_finish_supers(const double* sup, long long nsup, long long maxsup, int nranks, int nv,
                                double* out, hipStream_t s);
// Gauss-Newton moments of the accepted correspondences of [p0, p1) at T0 (R = rot(T0 * guess),
// ctr = expansion centre): chunk partials of kMomVals doubles (grid: chunk_grid_blocks)
int        chunk_grid_blocks(size_t ns);
hipError_t launch_gn_moments(const float4* src, const float4* tpts, const Cov3& cov_s,
                             const Cov3& cov_t, Rot33d R, Xf34 T0, const double ctr[3],
                             const uint32_t* nn_pos, const uint32_t* flags, size_t p0, size_t p1,
                             double* partial, int nb, hipStream_t s);
// n (<= 64) doubles -> mapped host memory, then seq -> the host-polled completion word
hipError_t launch_publish(const double* in, int n, double* host_out, unsigned long long* flag,
                          unsigned long long seq, hipStream_t s);
// fitness chunk partials ([0] sum d2, [13] count) of [p0, p1) (grid: chunk_grid_blocks)
hipError_t launch_fitness(const GridView& tgt, const float4* src, size_t p0, size_t p1,
                          Xf34 T, double max_range, double* partial, int nb, hipStream_t s);
hipError_t launch_reduce_finish(const double* partial, int nb, double* out, hipStream_t s);
hipError_t launch_resolution(const GridView& g, size_t n, double* partial, int nb, hipStream_t s);
hipError_t launch_radius_keep(const GridView& g, size_t n, float r2, int need, unsigned char* keep,
                              hipStream_t s);

// ---- FOD-side callers ----
// finite points of `in` -> out (order kept, w = original index kept); flags/pos: n + 1 each,
// scratch: scan_scratch_bytes(n + 1); the count is pos[n]
hipError_t launch_finite_compact(const float4* in, size_t n, uint32_t* flags, uint32_t* pos,
                                 void* scratch, size_t scratch_bytes, float4* out, hipStream_t s);
// SegmentDifferences: keep[i] = finite(T in_i) && 1-NN float d2 > thr; *count += kept
hipError_t launch_segdiff(const GridView& g, const float4* in, size_t n, Xf34 T, int has_T, double thr,
                          unsigned char* keep, unsigned int* count, hipStream_t s);
// VoxelGrid: leaf keys (non-finite -> 0xffffffff), run heads of the sorted keys (n + 1 flags),
// per-leaf centroids at the scanned head positions, min_points_per_voxel compaction
hipError_t launch_voxel_keys(const float4* pts, size_t n, const float inv[3], const int min_b[3],
                             int mul1, int mul2, uint32_t* keys, hipStream_t s);
hipError_t launch_voxel_heads(const uint32_t* keys_sorted, size_t n, uint32_t* flags, hipStream_t s);
hipError_t launch_voxel_centroids(const uint32_t* keys_sorted, const uint32_t* perm, const uint32_t* flags,
                                  const uint32_t* pos, size_t n, const float4* pts, const uint32_t* rgba,
                                  float4* out, uint32_t* out_rgba, hipStream_t s);
hipError_t launch_voxel_minpts(const float4* vox, const uint32_t* vox_rgba, size_t nv, uint32_t need,
                               uint32_t* flags, uint32_t* pos, void* scratch, size_t scratch_bytes,
                               float4* out, uint32_t* out_rgba, hipStream_t s);

// EuclideanClusterExtraction (FODDetector::clusterPossibleFODs): connected components of "float d2 < r2"
// over a grid whose cell edge is at least tolerance / 2.  launch_cc_link starts the union-find forest
// parent[n] (sorted positions) and, with `link`, unites every linked pair; shortcut = 1 promises that
// any two points of one cell are linked (they are united without a distance test).  *pair_tests
// (zeroed by the caller) += distance evaluations.  launch_cc_labels then writes, at each point's rank
// in original order (perm), keys = the smallest original index of its component, vals = its own.
hipError_t launch_cc_link(const GridView& g, size_t n, const uint32_t* keys_sorted, float r2, int shortcut, int link,
                          uint32_t* parent, unsigned long long* pair_tests, hipStream_t s);
hipError_t launch_cc_labels(const GridView& g, const uint32_t* perm, size_t n, uint32_t* parent, uint32_t* root,
                            uint32_t* min_orig, uint32_t* keys, uint32_t* vals, hipStream_t s);

// NormalEstimation with a radius search (Utils::getNormals): for every grid point, over its neighbours
// "float d2 < r2" (itself included), the normal (x, y, z) and curvature (w) of out[original index] and
// their number in count[original index]; fewer than 3: four NaNs.  out / count hold one entry per
// original record (the caller presets those of records outside the grid).  *pair_tests (zeroed by the
// caller) += distance evaluations.  Exact for any cell edge; fastest with an edge near the radius.
hipError_t launch_normals_tile(const GridView& g, size_t n, float r2, const float vp[3], float4* out, int* count,
                               unsigned long long* pair_tests, hipStream_t s);

// BoundaryEstimation with a k-search (InitialAlignment::obtainBoundaryKeypoints): for every grid point, over
// its k nearest grid points in (float d2, original index) order (itself included), the largest cyclic gap of
// the tangent-plane angles in gap[original index] and gap > thr in flag[original index]; records that are
// never boundary points keep the caller's presets (0 / NaN).  normals: 3 floats per original record.
// nn (nullable, preset to -1): k original indices per original record, in that order.  fb / fb_count
// (n entries / one zeroed counter): the queries the per-lane kernel hands to the wave-per-query one.
// *pair_tests (zeroed by the caller) += distance evaluations.  k in [1, 32].
hipError_t launch_boundary(const GridView& g, size_t n, const float* normals, int k, float thr, uint8_t* flag,
                           float* gap, int* nn, uint32_t* fb, unsigned int* fb_count,
                           unsigned long long* pair_tests, hipStream_t s);

// FPFHEstimation with a radius search (InitialAlignment::obtainFeatures), three steps over a grid of n
// finite points.  kp: nk original record indices in [0, records) (nullptr: 0 .. nk - 1).  Buffers by sorted
// position: mark / pos (n + 1 words), list (n), rows (n * 33 bin counts), msize (n set sizes; rows and msize
// zeroed by the caller); pos_of: one word per original record, preset to 0xffffffff.
// mark: pos_of, the members of every keypoint's set "float d2 < r2" marked and listed; the number of
// listed records lands in pos[n].  spfh: the SPFH bin counts and set size of every listed record
// (*too_big, zeroed by the caller, = 1 when a set -- a keypoint's in mark, a row's in spfh -- exceeds
// 65535; the steps after that leave their work undone: the call fails).  final: the weighted, normalised
// histogram of every keypoint, 33 floats each, NaN for a record outside the grid.
// ctr (2 * kFpfhCtrSlots words, zeroed by the caller): pairs of {distance evaluations, pair features};
// the totals are the sums over the slots.
constexpr int kFpfhCtrSlots = 256;
hipError_t launch_fpfh_mark(const GridView& g, size_t n, const int* kp, size_t nk, float r2, uint32_t* pos_of,
                            uint32_t* mark, uint32_t* pos, uint32_t* list, void* scratch, size_t scratch_bytes,
                            unsigned int* too_big, unsigned long long* ctr, hipStream_t s);
hipError_t launch_fpfh_spfh(const GridView& g, size_t n, const uint32_t* list, const uint32_t* count,
                            const float* normals, float r2, uint16_t* rows, int* msize, unsigned int* too_big,
                            unsigned long long* ctr, hipStream_t s);
hipError_t launch_fpfh_final(const GridView& g, const int* kp, size_t nk, const uint32_t* pos_of, float r2,
                             const uint16_t* rows, const int* msize, const unsigned int* too_big, float* out,
                             unsigned long long* ctr, hipStream_t s);

// HarrisKeypoint3D with a radius search (InitialAlignment::obtainHarrisKeypoints) over a grid of n finite
// points.  response: the normals (3 floats per original record) packed into nrm (n, grid order); for every
// grid point, over its set "float d2 < r2", the normal moments and the Harris response, into resp_pos (by
// sorted position) and, each nullable and preset by the caller for records outside the grid, resp_orig,
// covar (6 floats) and count by original index.  nms: flag[original index] = 1 (flag zeroed by the caller)
// for every point with a finite response not below thr that no member of its set exceeds.  compact: the
// flagged original indices, ascending, into list; their number lands in pos[records] (flag / pos:
// records + 1 words, flag[records] = 0).  fb / fb_count (n entries / one counter): the records a lane hands
// to the wave-per-record launch.  ctr (3 * kHarCtrSlots words, zeroed by the caller): triples of
// {distance evaluations, candidates, tied keypoints}; the totals are the sums over the slots.
constexpr int kHarCtrSlots = 256;
hipError_t launch_harris_response(const GridView& g, size_t n, const float* normals, float4* nrm, float r2, float thr,
                                  float* resp_pos, float* resp_orig, float* covar, int* count, uint32_t* fb,
                                  unsigned int* fb_count, unsigned long long* ctr, hipStream_t s);
hipError_t launch_harris_nms(const GridView& g, size_t n, const float* resp_pos, float r2, float thr, uint32_t* flag,
                             uint32_t* fb, unsigned int* fb_count, unsigned long long* ctr, hipStream_t s);
hipError_t launch_harris_compact(const uint32_t* flag, uint32_t* pos, size_t records, void* scratch,
                                 size_t scratch_bytes, uint32_t* list, hipStream_t s);

// CorrespondenceEstimation over 33-float descriptors (InitialAlignment::obtainCorrespondences): exact brute
// force.  src / tgt: ns / nt packed rows of 33 finite floats.  A source row's state is the key
// (d2 bits << 32) | (target row << 1) | tied, kMatchNone before any target with d2 < FLT_MAX; keys order as
// (d2, target row).  launch_match folds target rows [t_begin, t_end) into running[ns]: call it over
// ascending ranges, at most pairs_per_launch / ns rows each, so that no launch is long.  partial:
// match_layout(ns, rows of the largest range).splits * ns keys (unused when that is 1).
// ctr (3 words, zeroed by the caller) += pairs left at the votes after bins 8, 16 and 24.
constexpr uint32_t kMatchBlock = 256;            // threads = source rows of a block
constexpr uint32_t kMatchSplitMin = 64;          // target rows of a block: a multiple of this
constexpr uint32_t kMatchBlocksWanted = 8192;    // four rounds of 8 blocks per CU: the CUs' loads even out
constexpr uint32_t kMatchNoneLow = 0xfffffffeu;  // row field 0x7fffffff (no row: n <= INT32_MAX), not tied
constexpr unsigned long long kMatchNone = (0x7f7fffffull << 32) | kMatchNoneLow;  // d2 = FLT_MAX
// pairs of one launch: 13 ms at the 6.0e11 pairs/s measured on the README's 198k x 198k shape, where the
// votes leave 14 % of the pairs; about 20 ms at the 4.6e11 pairs/s of random rows, where they leave 7 %
// (DESIGN.md "Feature correspondences")
constexpr unsigned long long kMatchPairsPerLaunch = 1ull << 33;
struct MatchLayout {
  uint32_t splits;     // blocks that share the target rows of a launch (grid.y)
  uint32_t per_split;  // target rows of each
};
MatchLayout match_layout(size_t ns, size_t count);
hipError_t launch_match(const float* src, size_t ns, const float* tgt, size_t t_begin, size_t t_end,
                        unsigned long long* running, unsigned long long* partial, unsigned long long* ctr,
                        hipStream_t s);

// The rejectors and the SVD estimate of the pre-alignment (InitialAlignment::rejectCorrespondences,
// rejectOneToOneCorrespondences, estimateTransform) over m correspondences (iq[i], im[i]) between two
// keypoint clouds held as packed xyz; the caller has checked every index against its cloud.
struct PairView {
  const float* sxyz;  // 3 floats per source record
  const float* txyz;  // 3 floats per target record
  const int* iq;      // m source record indices
  const int* im;      // m target record indices
};
constexpr int kRansacBatch = 64;  // models of one scoring launch
// score: counts[b] (kRansacBatch words, zeroed here) = correspondences with float d2 < lim under model b of
// the nb (<= kRansacBatch) models, 12 floats each (the rows of a 3 x 4).  select: flag / pos (m + 1 words),
// d2 (m); the inliers' positions ascending in list and their d2 in d2_packed, their number in pos[m].
// moments: the 15 sums of pair_moments_kernel over list[0 .. cnt) (nullptr: 0 .. cnt) into out[16];
// partial: pair_moment_blocks(cnt) * kRedVals doubles.
hipError_t launch_ransac_score(const PairView& v, size_t m, const float* models, int nb, float lim,
                               unsigned int* counts, hipStream_t s);
hipError_t launch_ransac_select(const PairView& v, size_t m, Xf34 T, float lim, uint32_t* flag, uint32_t* pos,
                                float* d2, void* scratch, size_t scratch_bytes, uint32_t* list, float* d2_packed,
                                hipStream_t s);
int        pair_moment_blocks(size_t cnt);
hipError_t launch_pair_moments(const PairView& v, const uint32_t* list, size_t cnt, double* partial, double* out,
                               hipStream_t s);
// one-to-one: order[0 .. pos[nt]) = per target with a correspondence, ascending, the position of its
// smallest (dist, position); the rest of order[m] = -1.  im[i] < 0 is skipped, every other im[i] < nt;
// dist non-negative, no NaN, no -0.  best: max(nt, 1) words; flag / pos: nt + 1; scratch for nt + 1
hipError_t launch_one_to_one(const int* im, const float* dist, size_t m, size_t nt, unsigned long long* best,
                             uint32_t* flag, uint32_t* pos, void* scratch, size_t scratch_bytes, int* order,
                             hipStream_t s);

// Normal clustering (InitialAlignment::obtainNormalsCluster) over a grid of n finite points: PCL's serial
// rounds, each the closure of its seed.  begin: owner[n] = free, order[rank in original order] = sorted
// position, the normals (3 floats per original record) packed into nrm (n, grid order).  small: one
// workgroup runs consecutive rounds from state->cursor until the cursor passes n or a round holds more than
// `limit` (1 .. kNcSmallCap) records after a level; that round's frontier is then spill[0 .. state->count)
// and expand continues it, one launch per level: frontier[0 .. count) -> next / counts[parity]; counts (two
// words, both zero when a round's first level is launched) alternate: a launch zeroes counts[parity ^ 1].
// ctr (kNcCtrSlots words, zeroed by the caller) += candidates walked by expand; small adds its own to the
// state.  emit: (owner, original index) at each record's rank in original order, for the stable sort.
struct NcState {
  uint32_t cursor, status, seed, seed_pos, count, rounds;
  unsigned long long walked;
};
constexpr uint32_t kNcSmallCap = 4096;   // records of a round the small path can hold (its LDS frontiers)
constexpr uint32_t kNcSmallLimit = 256;  // records above which a round goes wide (debug option "nc_small_limit")
constexpr int kNcCtrSlots = 256;
hipError_t launch_nc_begin(const GridView& g, const uint32_t* perm, size_t n, const float* normals, float4* nrm,
                           uint32_t* owner, uint32_t* order, hipStream_t s);
hipError_t launch_nc_small(const GridView& g, size_t n, const float4* nrm, const uint32_t* order, uint32_t* owner,
                           float r2, float c_min, uint32_t limit, uint32_t* spill, NcState* state, hipStream_t s);
hipError_t launch_nc_expand(const GridView& g, const float4* nrm, uint32_t* owner, const uint32_t* frontier,
                            uint32_t count, float r2, const float seed_normal[3], float c_min, uint32_t seed,
                            uint32_t* next, unsigned int* counts, int parity, unsigned long long* ctr, hipStream_t s);
hipError_t launch_nc_emit(const GridView& g, const uint32_t* perm, size_t n, const uint32_t* owner, uint32_t* keys,
                          uint32_t* vals, hipStream_t s);
// Dominant normals (InitialAlignment::obtainDominantNormals): out[3 c] = the normalised fp64 sum of cluster
// c's entries (its first member, then every member) in the tree of launch_pair_moments taken per cluster.
// blk_cluster[n_blocks]: the cluster of every block of 256 entries; blk_first[n_clusters + 1]: a cluster's
// first block; partial: n_blocks * kRedVals doubles.
hipError_t launch_dominant_normals(const float* normals, const int* indices, const unsigned long long* offsets,
                                   const uint32_t* blk_cluster, const uint32_t* blk_first, size_t n_blocks,
                                   size_t n_clusters, double* partial, float* out, hipStream_t s);

#if defined(MGICP_CORR_PHASES) && MGICP_CORR_PHASES
hipError_t corr_phase_take(unsigned long long out[24]);  // diagnostic builds: read and reset
#endif
#if defined(MGICP_CORR_STATS) && MGICP_CORR_STATS
hipError_t corr_stats_take(unsigned long long out[8]);  // diagnostic builds: read and reset
#endif

// radix sort / scan scratch (hipcub)
size_t sort_scratch_bytes(size_t n, int bits);
hipError_t launch_sort_pairs(void* scratch, size_t scratch_bytes, const uint32_t* keys_in,
                             uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                             size_t n, int bits, hipStream_t s);
size_t scan_scratch_bytes(size_t n);
hipError_t launch_exclusive_scan(void* scratch, size_t scratch_bytes, const uint32_t* in,
                                 uint32_t* out, size_t n, hipStream_t s);
hipError_t launch_iota(uint32_t* v, size_t n, hipStream_t s);
// r05 target cache: *diff = 1 when a[0..n) and b[0..n) differ in any bit (else 0)
hipError_t launch_equal(const float4* a, const float4* b, size_t n, unsigned int* diff, hipStream_t s);
// resolve all kernels once (moves the code-object loading cost into mgicp_create)
// and exercise both copy directions once, small and large (pinned: pinned host scratch)
hipError_t preload_kernels(void* pinned, size_t pinned_bytes, hipStream_t s);
// empty-space distance map of a grid (3 separable capped min-max passes); scratch: nc bytes
hipError_t launch_empty_map(const uint32_t* cell_start, int nx, int ny, int nz, uint8_t* out,
                            uint8_t* scratch, hipStream_t s,
                            uint32_t* seed = nullptr /*nullable: nc entries*/, uint32_t* seed_scratch = nullptr,
                            const GridView* g = nullptr /*with seed: each cell's point nearest its centre*/);

}  // namespace mgicp
