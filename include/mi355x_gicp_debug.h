/*
 * mi355x_gicp_debug.h -- test, benchmark and diagnostic entry points of libmgicp.so.
 *
 * For the project's tests, bench.py and diagnostics only.  NOT part of the drop-in: an integrator
 * includes mi355x_gicp.h alone, and nothing the adapter calls is declared here.  These calls read the
 * engine's intermediate state (covariances, correspondences, partial sums, counters), time single
 * kernels, and switch one context between the engine's forms (mgicp_debug_option); they may change
 * with the engine's internals.
 */
#ifndef MI355X_GICP_DEBUG_H
#define MI355X_GICP_DEBUG_H

#include "mi355x_gicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- introspection for parity tests (original point order) ---- */
/* covariances of the source (which = 0) or target (which = 1): n x {c00,c01,c02,c11,c12,c22} */
int mgicp_debug_covariances(mgicp_ctx* ctx, int which, double* out_c6);
/* r06: the original indices of this rank's source points in the order the objective's compacted streams
 * -- and so every pass's fixed reduction tree -- visit them (the grid-sorted order); returns the count.
 * The oracle's summation-order ledger runs the engine's tree over it (oracle/gicp_ref.h ref_set_sum_order). */
int mgicp_debug_source_order(mgicp_ctx* ctx, uint32_t* out, size_t cap);
/* one correspondence sweep at T (col-major); out_tgt[i] = target index or -1;
 * out_M6 (optional) = n x {m00,m01,m02,m11,m12,m22}; returns the count or < 0 */
int mgicp_debug_correspondences(mgicp_ctx* ctx, const float T_cm[16], int* out_tgt, double* out_M6);
/* the same sweep SEEDED with the previous sweep's matches, as the outer iterations after the first
 * run it; same outputs */
int mgicp_debug_correspondences_seeded(mgicp_ctx* ctx, const float T_cm[16], int* out_tgt, double* out_M6);
/* OptimizationFunctorWithIndices::fdf at x over the last correspondence sweep */
int mgicp_debug_fdf(mgicp_ctx* ctx, const double x[6], double* f, double g6[6]);
/* the raw reduced sums of one objective pass at x: [0] sum r'Mr, [1..3] sum Mr,
 * [4..12] sum s (Mr)' row-major, [13] correspondence count.  With mgicp_comm_init(ctx, n, r,
 * NULL) (a "detached" shard, no RCCL) they cover rank r's source range only, so sharding can
 * be verified on one device; align/fitness refuse to run in that mode. */
int mgicp_debug_fdf_sums(mgicp_ctx* ctx, const double x[6], double out16[16]);
/* n objective passes at the states xs[6 k .. 6 k + 5] as ONE BFGS run makes them: a single resident
 * server (when the shard is servable) launched with the first pass, commanded n times and cancelled
 * after the last, so passes 2 .. n run on a live server with its chunks resident and its host rows
 * alternating between the two parity buffers (mgicp_debug_fdf_sums tears the server down after its
 * one pass).  out16n[16 k ..]: the sums of pass k, as mgicp_debug_fdf_sums.  1 <= n <= 4096. */
int mgicp_debug_fdf_sums_run(mgicp_ctx* ctx, const double* xs, int n, double* out16n);
/* Objective-pass timing (bench.py's roofline leg): npasses passes at state x over the last
 * correspondence sweep, back to back on the device, bracketed by HIP events on the context's
 * stream.  mode 0: the resident pass server (one launch running all passes; the pass
 * the aligns use on one GPU), mode 1: one fdf_soa_kernel launch per pass.  out_ms: average per
 * pass; out16: the sums of the last pass (as mgicp_debug_fdf_sums).  Single-rank contexts only. */
int mgicp_debug_pass_bench(mgicp_ctx* ctx, const double x[6], int npasses, int mode, double* out_ms,
                           double out16[16]);
/* MGICP_SOLVER_GN's moment pass at T (col-major) over the last correspondence sweep
 * (mgicp_debug_correspondences or an align): out80[0] sum r'Mr, [1..12] sum (Mr) w' (row-major
 * 3x4), [13..72] sum M_p (w w')_q (p: m00 m01 m02 m11 m12 m22; q: upper triangle of the 4x4
 * w w'), [73] count, with r = fl(fl(T s) - q), w = (s - c, 1), c = bbox midpoint of the source */
int mgicp_debug_moments(mgicp_ctx* ctx, const float T_cm[16], double out80[80]);
/* The fixed reduction tree behind every sharded sum (objective passes, GN moments, fitness):
 * chunks of 1024 grid-sorted source positions, supers of 32 chunks, then a fixed-order total over
 * the supers; rank r of N owns supers [nsup * r / N, nsup * (r + 1) / N), so its super partials are
 * the single-GPU run's, bit for bit.  mgicp_debug_supers writes this shard's super partials of one
 * pass -- kind 0: objective pass at x = arg[0..5] (16 values per super, as mgicp_debug_fdf_sums);
 * kind 1: the GN moment pass at the col-major T = arg[0..15] (80 per super, as
 * mgicp_debug_moments); kind 2: getFitnessScore at T = arg[0..15], max_range = arg[16] (16 per
 * super: [0] sum d2, [13] count) -- and returns how many (<= cap) or < 0. */
int mgicp_debug_supers(mgicp_ctx* ctx, int kind, const double* arg, double* out, int cap);
/* the multi-GPU finish itself: the fixed-order total of nsup supers of nv (16 or 80) values held as
 * nranks rows of maxsup supers (row r = rank r's supers; padding rows are never read) */
int mgicp_debug_finish_supers(mgicp_ctx* ctx, int nv, const double* rows, long long nsup, long long maxsup,
                              int nranks, double* out);
/* the chunk reduction of every pass (one wave, 16 values per lane): for each of nwaves waves of
 * in[w][lane][16], out_tree[w][16] = 16 wave_sum shuffle trees (lane 0's sums) and out_rs[w][16] =
 * the register reduce-scatter the passes use (permlane swaps + DPP); the two must agree bit for bit */
int mgicp_debug_wave_reduce(mgicp_ctx* ctx, const double* in, int nwaves, double* out_tree, double* out_rs);
/* per-iteration transformation_ of the last align (col-major, iterations x 16) */
int mgicp_debug_trace(mgicp_ctx* ctx, float* out, int max_iters);
/* average device time (ms) of each kernel family while profiling is on, for roofline
 * reporting: [0] covariance kNN, [1] correspondence 1-NN, [2] BFGS objective pass,
 * [3] separate reduction finish, [4] compaction + Mahalanobis, [5] Gauss-Newton moment pass (+ its
 * finish); counts in out_counts (optional) */
#define MGICP_KERNEL_FAMILIES 6
int mgicp_debug_kernel_times(mgicp_ctx* ctx, double out_ms[MGICP_KERNEL_FAMILIES],
                             int out_counts[MGICP_KERNEL_FAMILIES]);
/* objective-pass path counters since mgicp_create: [0] resident servers launched, [1] passes run
 * by a server, [2] passes run by launched kernels, [3] server passes that missed their deadline
 * (env MGICP_ROW_DEADLINE_MS, default 500) and were taken over by a launched pass (bitwise the
 * same sums; the rest of that align runs launched passes), [4] 1 if the server reads its commands
 * from device memory the host writes through the BAR, [5] private host-row buffer allocations,
 * [6] transport (0 local, 1 RCCL, 2 shared segment, 3 shared segment + RCCL, 4 xGMI row exchange
 * over the segment, 5 xGMI row exchange + RCCL), [7] server launches
 * refused because another context of this process ran a server on the same device, [8] objective
 * evaluations answered without a pass: their fp32 transform had been passed over in the same BFGS
 * run (debug option "pass_memo"), so [1] + [2] - [3] + [8] is what n_evals would be without */
int mgicp_debug_pass_stats(mgicp_ctx* ctx, long long out[9]);
/* correspondence rounds of the BFGS mode since mgicp_create (debug option "round_fast"): [0] fast rounds
 * -- a fused listed sweep whose counters came back zero, so nothing followed its query kernel -- [1] slow
 * rounds (every other round: cold or unfused sweeps, and fused ones with work left), [2] fused rounds
 * that deferred chunks to the compaction launch, [3] fused rounds that left queries pending.  [2] and
 * [3] are known only where the counters are read, i.e. with "round_fast" 1. */
int mgicp_debug_round_stats(mgicp_ctx* ctx, long long out[4]);
/* the resident pass server as the aligns run it (always on, two HIP events per server launch on the
 * engine's stream, resolved when an align drains): *out_ms = summed device duration of the server
 * launches (first command .. cancel, host round trips between passes included), *out_passes = the
 * passes those launches ran, *out_launches = the launches; reset = 1 zeroes the counters after the
 * read.  out_ms / out_passes = the in-align time of one objective pass. */
int mgicp_debug_server_time(mgicp_ctx* ctx, double* out_ms, long long* out_passes, long long* out_launches,
                            int reset);
/* the r-th of N target-covariance slices exactly as rank r of an N-rank context computes it before
 * the all-gather (points [r cnt, min(n, (r + 1) cnt)), cnt = ceil(n / N), arrays of N cnt entries):
 * 6 values per point of the slice, in grid-sorted order, into out_c6 (c00 c01 c02 c11 c12 c22);
 * returns the slice's point count.  Assembled in rank order the N slices are the all-gathered arrays (tests; the cached target
 * covariances are recomputed by the next align). */
int mgicp_debug_target_cov_slice(mgicp_ctx* ctx, int nranks, int rank, double* out_c6);
/* the target's 1-NN cell lists (DESIGN.md "1-NN cell lists"): out[0] cells requested and out[1]
 * queries left to the exact per-lane search by the last sweep, out[2] cells with a list, out[3] list
 * entries, out[4] reject cells, out[5] overflow cells, out[6] pool entries used, out[7] fine-grid
 * cells (0 when the lists are off: debug option "vlist" 0 or a gate too wide for a fine grid) */
int mgicp_debug_vlist_stats(mgicp_ctx* ctx, long long out[8]);
/* the fine grid of those lists, its counters and (optionally) every fine cell, computed on the host from
 * copies of the state words, the counters and the long lists' header entries (no kernel runs):
 * out[0..2] grid origin ox oy oz, out[3] cell edge c, out[4] es (growth of a cell's box covering the fp32
 * cell assignment), out[5..7] nx ny nz, out[8] the gate, out[9] the target grid's cell edge h, out[10] 1
 * when the gate is too wide for a fine grid (lists off: out[0..7] and all that follows are 0), out[11]
 * pool capacity and out[12] pool head (entries; the head may pass the capacity, no list lies beyond it),
 * out[13] slots of the build list, out[14] cells requested, out[15] queries pending and out[16] cells
 * handed to the build's second pass by the last sweep, out[17] fine-grid cells (cell i = ix + nx (iy +
 * ny iz)), out[18] 1 once the state words and the pool are allocated (else out[11..16] are 0 and no cell
 * is written), out[19] the float reciprocal of c the queries' cell assignment multiplies by, out[20..23]
 * 0.  state / length / offset (each optional, `cap` >= out[17] elements): per fine cell its class (0 not
 * built, 1 touched, 2 requested, 3 reject, 4 overflow, 5 listed), its list's true length (a long list's
 * from its header entry) and the list's first pool entry (a long list's header; the list occupies
 * length rounded up to a multiple of 4, + 4 for a long list's header). */
int mgicp_debug_vlist_layout(mgicp_ctx* ctx, double out[24], uint8_t* state, uint32_t* length, uint32_t* offset,
                             size_t cap);
/* the last mgicp_match_features call on this context (DESIGN.md "Feature correspondences"): out[0] pairs
 * begun, out[1..3] pairs left at the wave votes after bins 8, 16 and 24, out[4] launches of the match
 * kernel, out[5] target rows of a launch, out[6] blocks that share them and out[7] target rows of each
 * such block (the layout of the first launch); all 0 when the call ran no kernel */
int mgicp_debug_match_stats(mgicp_ctx* ctx, long long out[8]);
/* the scoring kernel of mgicp_reject_ransac on caller-given models: counts[b] = the correspondences whose
 * float d2 under models_cm[b] (column-major 4 x 4, the last row ignored) satisfies (double)d2 < threshold *
 * threshold -- the distance rule of mi355x_gicp.h "the pre-alignment transform".  n_models >= 0, any number:
 * scored in launches of up to 64 (or the "ransac_batch" option's value).  Arguments checked as
 * mgicp_reject_ransac checks them. */
int mgicp_debug_score_models(mgicp_ctx* ctx,
                             const float* source_keypoints, size_t n_source, size_t source_stride_bytes,
                             const float* target_keypoints, size_t n_target, size_t target_stride_bytes,
                             const int* index_query, const int* index_match, size_t m,
                             const float* models_cm /* n_models * 16 */, int n_models, double threshold,
                             int* counts /* n_models */);
/* enable (1) / disable (0) per-launch HIP event timing (off by default); objective passes
 * ([2]) are sampled every 8th launch, every other family is timed on every launch */
int mgicp_set_profiling(mgicp_ctx* ctx, int on);
/* test / diagnostic forms of the engine, set explicitly on one context (never through the
 * environment): "resident", "host_rows", "srv_cus", "fused_finish", "gated", "bar_cmd" (the
 * objective-pass path), "async_cov", "lazy_src_cov", "knn_logged", "knn_wave" (covariances), "vlist",
 * "vlist_cold", "vlist_eager", "vlist_stats", "vlist_pool" (a list pool of max(N, 4096) entries instead of
 * the default max(2^22, 32 n); 0: the default; such a context leaves no lists in the target cache),
 * "fuse_compact" (1-NN cell lists),
 * "target_cache", "match_pairs_per_launch" (mgicp_match_features: the (source, target) pairs of one launch;
 * 0: the default), "ransac_batch" (mgicp_reject_ransac: the hypotheses of one scoring launch, 1 .. 64;
 * 0: the default of 64), "nc_small_limit" (mgicp_normal_clusters: the records above which a round leaves the
 * one-workgroup path for the level-synchronous one, 1 .. 4096; 1: every multi-record round; 0: the default of
 * 256).  Every form gives the default path's results bit for bit (the GPU tests
 * that pin each one: INTEGRATION.md "Debug options"); MGICP_E_INVALID for an unknown name. */
int mgicp_debug_option(mgicp_ctx* ctx, const char* name, double value);
/* target cache (mgicp_release_cache): out[0] the current target was adopted from the cache, out[1]
 * adoptions and out[2] donations on this device so far, out[3] an entry is cached on this device,
 * out[4] 0 (r05: the source grid's start from a cached target; since r06 a grid depends on its own cloud
 * alone).
 * Debug option "target_cache" 1: this context adopts and leaves targets (default 0: neither). */
int mgicp_debug_cache_stats(mgicp_ctx* ctx, long long out[5]);

#ifdef __cplusplus
}
#endif
#endif
