/*
 * mi355x_gicp.h -- C-ABI of the MI355X-native GICP fine-alignment engine (libmgicp.so).
 *
 * This is the drop-in boundary for the reference's hot path
 *     GICPAlignment::fineAlignment()  ->  gicp_.align(*aligned_cloud)
 *     (/root/reference/src/GICPAlignment.cpp:86-109, the align call at :96, and the
 *      second align in iterateFineAlignment at :116)
 * i.e. it replaces pcl::GeneralizedIterativeClosestPoint<PointXYZRGB,PointXYZRGB>
 * (/root/reference/include/GICPAlignment.h:153) under the unchanged GICPAlignment class.
 * Plain pointers and sizes only; no PCL, Eigen, HIP or torch types cross this header.
 *
 * Matrices are 4x4 float, COLUMN-MAJOR (Eigen::Matrix4f storage order).
 * Point clouds are passed as xyz at byte offsets 0/4/8 of records of `stride_bytes`
 * (32 for pcl::PointXYZRGB, 16 for pcl::PointXYZ, 12 for packed xyz).
 *
 * Threading: one context per host thread; every call blocks until its result is on the
 * host.  Several contexts may align on one device at once: one of them at a time runs the
 * resident pass server (it needs every CU), the others run launched passes.  Status codes: 0 = OK,
 * negative = error (mgicp_last_error() has the message).
 */
#ifndef MI355X_GICP_H
#define MI355X_GICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGICP_OK                0
#define MGICP_E_INVALID        -1  /* bad argument / state */
#define MGICP_E_TOO_FEW_POINTS -2  /* a cloud has fewer than k points (PCL logs and leaves
                                      its covariances empty, gicp.hpp computeCovariances) */
#define MGICP_E_SOLVER         -3  /* < 4 correspondences or BFGS failure: PCL's
                                      estimateRigidTransformationBFGS throws; align() returns
                                      this with converged = 0 and T = last good transform */
#define MGICP_E_NONFINITE      -4  /* NaN/Inf coordinates in an input cloud */
#define MGICP_E_HIP            -5  /* HIP runtime error */
#define MGICP_E_COMM           -6  /* RCCL error */
#define MGICP_E_NOMEM          -7  /* device allocation failed / grid too large */

#define MGICP_SOLVER_PCL_BFGS   0  /* PCL 1.8.1 BFGS trajectory (parity mode, default) */
#define MGICP_SOLVER_GN         1  /* opt-in fast mode (SURVEY.md 8b "solver"): one device pass
                                      per outer iteration collects the 74 moments of the
                                      quadratic objective, Gauss-Newton on SE(3) runs on the host;
                                      multi-GPU: one 80-double all-reduce per outer iteration.
                                      Not in PCL 1.8.1: reported against the fixed-point protocol
                                      and the oracle's GN restatement, not the BFGS trajectory */

typedef struct {
    int    max_iter;        /* Registration::setMaximumIterations  (GICPAlignment.cpp:50; default 100) */
    double tf_eps;          /* setTransformationEpsilon             (GICPAlignment.cpp:52; default 4e-3) */
    double rot_eps;         /* GICP rotation_epsilon_                (PCL default 2e-3) */
    double max_corr_dist;   /* setMaxCorrespondenceDistance          (GICPAlignment.cpp:51; default 0.04) */
    double gicp_eps;        /* GICP gicp_epsilon_                    (PCL default 1e-3; finite and >= 0, 0 legal as
                               in PCL: a NaN, negative or infinite value is refused with MGICP_E_INVALID) */
    int    k;               /* GICP k_correspondences_               (PCL default 20; any k in [1, 32]) */
    int    max_inner_iter;  /* GICP max_inner_iterations_            (PCL default 20) */
    int    solver;          /* MGICP_SOLVER_* */
    int    device;          /* HIP device ordinal; -1 = current device */
    int    fixed_iterations;/* 1 = ignore the delta test and run exactly max_iter iterations
                               (matched-iteration parity protocol) */
} mgicp_params;

typedef struct {
    int    converged;       /* Registration::hasConverged() */
    int    iterations;      /* GICP nr_iterations_ */
    int    n_corr;          /* correspondences in the last outer iteration (all ranks) */
    int    n_evals;         /* BFGS objective passes run over the correspondences (evaluations whose fp32
                               transform the run had already passed over take no pass and do not count) */
    double ms_total;        /* host call -> transform on host */
    double ms_upload;       /* host -> HBM copies of dirty clouds */
    double ms_prep;         /* grid build + kNN covariances (one-time per set_*) */
    double ms_loop;         /* outer GICP loop (correspondences + BFGS) */
} mgicp_result;

typedef struct mgicp_ctx mgicp_ctx;

/* ---- lifecycle ---- */
void        mgicp_default_params(mgicp_params* p);
int         mgicp_create(mgicp_ctx** ctx, const mgicp_params* p);
int         mgicp_set_params(mgicp_ctx* ctx, const mgicp_params* p);
const char* mgicp_last_error(const mgicp_ctx* ctx);
void        mgicp_destroy(mgicp_ctx* ctx);
/* r05 target cache (r06: OPT-IN per context, debug option "target_cache" 1 -- mgicp_debug_option,
 * declared in mi355x_gicp_debug.h; off by default because the
 * reference node aligns once per process): mgicp_destroy leaves such a single-rank context's target state
 * (grid, covariances, 1-NN cell lists; ~0.5-3 GB at 5M points) in a process-wide cache, one entry per
 * device; a later opted-in set_target whose points equal the cached ones bit for bit (compared on the
 * device) adopts it instead of rebuilding -- results are those of a rebuild bit for bit.  A device
 * allocation that runs out of memory evicts the device's entry and retries once.  This frees every
 * cached entry. */
void        mgicp_release_cache(void);
int         mgicp_device_count(int* n);

/* ---- inputs (Registration::setInputTarget / setInputSource) ----
 * At most 2^31 - 2 points per cloud (32-bit point indices); larger clouds return MGICP_E_INVALID.
 * Host buffers are copied at call time; the cloud is marked dirty so the next align()
 * rebuilds its grid and covariances (PCL resets its trees/covariances the same way).
 * The *_device variants take a device pointer already resident in HBM on this context's
 * device (no H2D copy).  Device buffers are copied at call time too: the engine packs the xyz
 * into its own storage before the call returns, never writes to the caller's buffer and never
 * reads it again, so the caller may overwrite or free it afterwards.  The pointer needs float
 * (4-byte) alignment only.  n = 0, a NULL pointer or a stride below 12 or not a multiple of 4
 * returns MGICP_E_INVALID before anything is launched. */
int mgicp_set_target(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes);
int mgicp_set_source(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes);
int mgicp_set_target_device(mgicp_ctx* ctx, const float* d_xyz, size_t n, size_t stride_bytes);
int mgicp_set_source_device(mgicp_ctx* ctx, const float* d_xyz, size_t n, size_t stride_bytes);

/* ---- the hot path: Registration::align(output, guess) ----
 * guess may be NULL (identity, as GICPAlignment calls align()).  out_T receives
 * getFinalTransformation().  Returns MGICP_E_SOLVER when PCL would report !hasConverged()
 * because the solver threw. */
int mgicp_align(mgicp_ctx* ctx, const float guess_cm[16], float out_T_cm[16], mgicp_result* res);

/* Registration::getFitnessScore(max_range) for transform T over the source cloud
 * (GICPAlignment.cpp:103,123).  max_range <= 0 means DBL_MAX (PCL default). */
int mgicp_fitness(mgicp_ctx* ctx, const float T_cm[16], double max_range, double* out);

/* pcl::transformPointCloud(source, out, T) for the xyz fields (GICPAlignment.cpp:144-147):
 * writes n transformed xyz triples into out (record stride out_stride_bytes), leaving the
 * other bytes of each record untouched.  Each coordinate is ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 in
 * float without FMA contraction; the last row of T is not read.  Every record goes through that
 * formula, non-finite ones included: NaN propagates and 0 * Inf = NaN.  (PCL skips non-finite
 * points of a non-dense cloud and leaves them as they are; this call does not -- that is the
 * contract.)  out_stride_bytes below 12 or not a multiple of 4: MGICP_E_INVALID. */
int mgicp_transform_source(mgicp_ctx* ctx, const float T_cm[16], float* out, size_t out_stride_bytes);

/* pcl::transformPointCloud(in, out, T) for any cloud (GICPAlignment::applyTFtoCloud,
 * src/GICPAlignment.cpp:144-147): xyz of n records of `in` are transformed on the GPU and
 * written into `out` (other bytes of the out records untouched; in == out allowed: `in`
 * is read whole before `out` is written).  The same float formula as mgicp_transform_source, applied to every record: NaN
 * propagates and 0 * Inf = NaN, where PCL would skip the non-finite points of a non-dense cloud.
 * Either stride below 12 or not a multiple of 4: MGICP_E_INVALID; n = 0: OK. */
int mgicp_transform_cloud(mgicp_ctx* ctx, const float T_cm[16], const float* in, size_t n,
                          size_t in_stride_bytes, float* out, size_t out_stride_bytes);

/* ---- helpers of GICPAlignment(use_covariances = true) ----
 * Utils::computeCloudResolution (src/Utils.cpp:145-174): mean distance from each point to its
 * nearest other point (the 2nd of a 2-NN query), fp64 sum of float sqrt.  Non-finite records are
 * skipped as queries and as neighbours (0 when fewer than 2 finite points remain). */
int mgicp_cloud_resolution(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                           double* out);
/* The NaN-normal removal of GICPAlignment::getCovariances (src/GICPAlignment.cpp:56-71):
 * pcl::NormalEstimation yields a NaN normal when fewer than 3 points (self included) lie
 * within the search radius (KdTreeFLANN::radiusSearch: float d^2 < float(radius^2)).
 * keep[i] = 1 iff record i is finite and at least min_neighbors finite points (itself included)
 * lie within the radius; non-finite records always get keep[i] = 0 (NaN normal). */
int mgicp_radius_filter(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                        double radius, int min_neighbors, unsigned char* keep);

/* Utils::getNormals (src/Utils.cpp:27-44; InitialAlignment.cpp:69-70 and GICPAlignment::getCovariances
 * call it): pcl::NormalEstimation<PointXYZRGB, Normal> with a radius search, PCL 1.8.1
 * computeFeature / computePointNormal restated.  The neighbour set of record i is every finite record
 * j (i included) with FLANN's float ((dx^2) + dy^2) + dz^2 < float(radius^2), strict -- the test of the
 * radius filter above; n_neighbors[i] is its size (exact; 0 for a non-finite record).  A non-finite
 * record, or one whose set holds fewer than 3 points, gets normal (NaN, NaN, NaN) and curvature NaN:
 * exactly the records with keep = 0 from mgicp_radius_filter(..., radius, 3, keep).  Otherwise: the
 * covariance C = S / m - mu mu' of the set from fp64 sums of the fp64 differences p_j - q_i, added in
 * grid order by one lane (the same bits every call; PCL's float raw moments about the origin in
 * FLANN's order are NOT reproduced, DESIGN.md "Radius normals"); the normal is the unit eigenvector
 * of C's smallest eigenvalue (fp64 Jacobi), the curvature |lambda_min / trace(C)| (0 when the trace is
 * 0); both are rounded to float and the normal is flipped when (viewpoint - q_i) . n < 0
 * (flipNormalTowardsViewpoint; viewpoint NULL: (0, 0, 0), PCL's default).  A set whose points are all
 * identical or collinear has no plane: its normal is NaN or some unit vector, no direction promised.
 * x, y, z go to byte offsets 0/4/8 of records of normal_stride_bytes (>= 12, a multiple of 4; 32 for
 * pcl::Normal, whose curvature at offset 16 the caller copies from the packed array), other bytes
 * untouched.  float(radius^2) = 0 links nothing: every record NaN, every count 0.  radius negative or
 * NaN, a bad pointer or stride: MGICP_E_INVALID; n = 0: OK.
 * Uses the helper cloud slot: a set source / target and their cached state stay as they are.
 * Single rank: with a communicator attached it runs locally, without a collective. */
typedef struct {
    double n_finite;     /* finite records (the searched tree) */
    double n_nan;        /* records that received a NaN normal */
    double pair_tests;   /* point-pair distance evaluations the device made */
    double ms_grid;      /* host call -> grid of the finite records built (upload included) */
    double ms_device;    /* first launch -> stream synchronise after the last */
    double ms_total;     /* host call -> outputs written */
} mgicp_normals_info;
int mgicp_estimate_normals(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                           double radius, const float viewpoint[3] /* NULL: (0,0,0) */,
                           float* normals, size_t normal_stride_bytes,
                           float* curvature /* may be NULL, packed n */,
                           int* n_neighbors /* may be NULL, packed n */,
                           mgicp_normals_info* info /* may be NULL */);

/* InitialAlignment::obtainBoundaryKeypoints (src/InitialAlignment.cpp:426-456; the BOUNDARY and NORMALS
 * methods call it on both clouds after getNormals): pcl::BoundaryEstimation<PointXYZRGB, Normal, Boundary>
 * with setKSearch(30) and setAngleThreshold(1.047f); PCL 1.8.1 computeFeature / isBoundaryPoint /
 * getCoordinateSystemOnPlane restated [PCL].
 * Neighbour set of record i: its k nearest FINITE records, itself included, by FLANN's float
 * ((dx^2) + dy^2) + dz^2; order and ties at the k-th distance go by (d2, original record index) -- the
 * engine's rule; FLANN's choice among equal distances depends on its tree and is not reproduced.  With
 * fewer than k finite records every finite record is in the set.  nn_indices[i * k ..] holds the set as
 * original record indices in that order, padded with -1; a non-finite record gets all -1.
 * Never a boundary point (max_gap = NaN, boundary = 0): a non-finite record; a record whose normal has a
 * non-finite component (deliberate: in PCL the NaN angles go through std::sort and the answer is "false"
 * in practice); a set of fewer than 3 records; a set in which every member has
 * delta = p_j - q_i = (0, 0, 0).  (A finite normal that still makes an angle NaN -- zero length, or
 * squares that overflow -- is treated like a non-finite one.)
 * Otherwise, all in float without FMA contraction: v = Eigen's generic unitOrthogonal of (n_x, n_y, n_z, 0)
 * (maxi = the first index of the largest |component|, sndi = maxi == 0 ? 1 : 0,
 * inv = 1 / sqrt(n[sndi]^2 + n[maxi]^2), v[maxi] = -n[sndi] inv, v[sndi] = n[maxi] inv, the rest 0),
 * u = n x v; for each member with delta != 0 the angle atan2f(v . delta, u . delta), dots summed as
 * (x + y) + z; the angles sorted ascending; max_dif starts at FLT_MIN and takes every consecutive
 * difference and the wrap (2 float(pi) - last) + first; max_gap[i] = max_dif and
 * boundary[i] = max_gap[i] > (float)angle_threshold.  PCL's SIMD dot order and its libm atan2f are not
 * pinned: the decision does not depend on the choice of (u, v) in exact arithmetic, so they matter at
 * rounding level only (DESIGN.md "Boundary estimation").
 * normals: x, y, z at byte offsets 0/4/8 of records of normal_stride_bytes (>= 12, a multiple of 4; 32
 * for pcl::Normal).  k outside [1, 32], a NaN threshold, a bad pointer or stride: MGICP_E_INVALID;
 * n = 0: OK; k < 3 is legal and flags nothing.  The same bits in every output on every call.
 * Uses the helper cloud slot: a set source / target and their cached state stay as they are.
 * Single rank: with a communicator attached it runs locally, without a collective. */
typedef struct {
    double n_finite;     /* finite records (the searched tree) */
    double n_boundary;   /* records flagged 1 */
    double n_undecided;  /* finite records that got max_gap = NaN (rules above) */
    double pair_tests;   /* point-pair distance evaluations the device made */
    double ms_grid;      /* host call -> grid of the finite records built (uploads included) */
    double ms_device;    /* first launch -> stream synchronise after the last */
    double ms_total;     /* host call -> outputs written */
} mgicp_boundary_info;
int mgicp_boundary_points(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                          const float* normals, size_t normal_stride_bytes,
                          int k, double angle_threshold,
                          unsigned char* boundary /* n, 0/1 */,
                          float* max_gap /* may be NULL, packed n */,
                          int* nn_indices /* may be NULL, n * k */,
                          mgicp_boundary_info* info /* may be NULL */);

/* InitialAlignment::obtainHarrisKeypoints (src/InitialAlignment.cpp:399-424; the HARRIS method calls it on
 * both clouds after getNormals): pcl::HarrisKeypoint3D<PointXYZRGB, PointXYZI> with its default method
 * HARRIS, setNonMaxSupression(true), setThreshold(1e-6), setRadius(radius_factor_ * resolution), refine off;
 * PCL 1.8.1 harris_3d.hpp (detectKeypoints, calculateNormalCovar, responseHarris) restated [PCL].  PCL is
 * not available to this project's tests, so parity with PCL binaries is unpinned (README "Parity"); the
 * rules below are the contract, and every deviation from PCL in them is deliberate.
 * Neighbour set N(i) of a finite record i: every finite record j, i included, with FLANN's float
 * ((dx^2) + dy^2) + dz^2 < float(radius^2), strict -- the set of mgicp_estimate_normals;
 * n_neighbors[i] = |N(i)| (exact; 0 for a non-finite record).  Non-finite records are in no set.
 * Normal moments (calculateNormalCovar): c_i = the members of N(i) whose normal_x is finite (PCL tests x
 * alone: a NaN or Inf in another component goes through the sums); for each of them the six products
 * nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, each rounded to float without FMA contraction.  Deviation (a):
 * the products are summed in fp64 in the engine's own fixed order (ascending grid position on a grid that
 * depends on the cloud and the radius alone) and covar = (float)(S / (double)c_i) -- PCL adds them in float
 * in FLANN's order and multiplies by float(1.0 / count).  c_i = 0: six zeros.  covar[i * 6 ..] = xx xy xz
 * yy yz zz; a non-finite record gets six zeros.
 * Response (responseHarris), in float without FMA contraction, PCL's expression left to right:
 * trace = (xx + yy) + zz; if trace != 0,
 * det = ((((xx yy) zz + ((2 xy) xz) yz) - (xz xz) yy) - (xy xy) zz) - (yz yz) xx and
 * response = (0.04f + det) - (0.04f trace) trace (the "0.04f +" is PCL's: it quantises det to the ulp of
 * 0.04, so equal responses are common); otherwise 0.  A non-finite record gets 0.
 * Keypoints, nonmax != 0: record i iff it is finite, response[i] is finite, !(response[i] < threshold) and
 * no j in N(i) has response[i] < response[j].  Equal responses keep both records; a NaN neighbour
 * suppresses nothing.  nonmax == 0: every record 0 .. n - 1 (PCL's branch returns the response cloud), the
 * second sweep is not run and n_tied is 0.  keypoints: the record indices ascending (deviation (b): PCL's
 * OpenMP order is not reproduced), *n_keypoints of them, the entries after those set to -1.
 * normals: x, y, z at byte offsets 0/4/8 of records of normal_stride_bytes (>= 12, a multiple of 4; 32
 * for pcl::Normal).  float(radius^2) = 0 links nothing: every response is 0 and no record is a keypoint for
 * a positive threshold.  radius negative or NaN, a NaN threshold, a bad pointer or stride, n > INT32_MAX:
 * MGICP_E_INVALID; n = 0: OK.  The same bits in every output on every call.
 * Uses the helper cloud slot: a set source / target and their cached state stay as they are.
 * Single rank: with a communicator attached it runs locally, without a collective. */
typedef struct {
    double n_finite;      /* finite records (the searched tree) */
    double n_candidates;  /* records with a finite response >= threshold */
    double n_keypoints;   /* indices written */
    double n_tied;        /* keypoints whose response is equalled by another member of their set */
    double pair_tests;    /* point-pair distance evaluations of both sweeps */
    double ms_grid;       /* host call -> grid of the finite records built (uploads included) */
    double ms_device;     /* first launch -> stream synchronise after the last */
    double ms_total;      /* host call -> outputs written */
} mgicp_harris_info;
int mgicp_harris_keypoints(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                           const float* normals, size_t normal_stride_bytes,
                           double radius, float threshold, int nonmax,
                           int* keypoints /* capacity n, ascending record index */, size_t* n_keypoints,
                           float* response /* may be NULL, packed n */,
                           float* covar /* may be NULL, n * 6: xx xy xz yy yz zz */,
                           int* n_neighbors /* may be NULL, packed n */,
                           mgicp_harris_info* info /* may be NULL */);

/* InitialAlignment::obtainFeatures (src/InitialAlignment.cpp:487-508; the BOUNDARY and HARRIS methods call it
 * at the keypoint indices, MULTISCALE's estimator is the same over every point):
 * pcl::FPFHEstimation<PointXYZRGB, Normal, FPFHSignature33> with setRadiusSearch(radius_factor_ * resolution);
 * PCL 1.8.1 fpfh.hpp (computeFeature, computeSPFHSignatures, computePointSPFHSignature,
 * weightPointSPFHSignature) and pfh_tools (computePairFeatures) restated [PCL].  PCL is not available to
 * this project's tests, so parity with PCL binaries is unpinned (README "Parity"); the rules below are
 * the contract, and every deviation from PCL in them is deliberate.
 * Neighbour set N(i) of a finite record i: every finite record j, i included, with FLANN's float
 * ((dx^2) + dy^2) + dz^2 < float(radius^2), strict (the test of mgicp_radius_filter); m_i = |N(i)|.
 * Non-finite records are in no set.
 * SPFH row of record i: for every j in N(i), j != i, computePairFeatures(p_i, n_i, p_j, n_j) in float
 * without FMA contraction, dots and squared norms summed as (x + y) + z: dp = p_j - p_i, f4 = |dp|; the
 * pair is skipped when f4 == 0; a1 = n_i . dp / f4, a2 = n_j . dp / f4; if acosf(|a1|) > acosf(|a2|)
 * the roles swap (n1 = n_j, n2 = n_i, dp = -dp, f3 = -a2), else n1 = n_i, n2 = n_j, f3 = a1;
 * v = dp x n1, the pair is skipped when |v| == 0, else v /= |v|; w = n1 x v; f2 = v . n2;
 * f1 = atan2f(w . n2, n1 . n2).  Bins, 11 per feature, the brackets in double as PCL's constants make
 * them: floor(11 ((f1 + M_PI) d_pi)) with the float d_pi = 1.0f / (2.0f * (float)M_PI),
 * floor(11 ((f2 + 1.0) 0.5)), floor(11 ((f3 + 1.0) 0.5)), each clamped to [0, 10].  A pair that is not
 * skipped adds one count to one bin of each feature.  Deviations: (a) the row is kept as integer counts
 * and its value is (float)count * (100.f / (float)(m_i - 1)), each rounded once -- PCL adds hist_incr
 * repeatedly in float, in FLANN's order; as in PCL, m_i - 1 counts skipped pairs too; (b) a pair in which
 * either normal has a non-finite component, or whose features come out NaN, is skipped -- in PCL it
 * reaches a float-to-int cast of NaN; (c) libm's acosf / atan2f are not pinned.  m_i = 1: a zero row.
 * Rows computed (computeSPFHSignatures): those of the union of N(q) over the keypoints q.
 * spfh_sizes[i] = m_i for them and 0 for every other record; spfh_counts[i * 33 ..] = the bin counts
 * (f1's 11, f2's 11, f3's 11), zero for every other record.
 * FPFH of keypoint q (weightPointSPFHSignature): bin b = sum over the j in N(q) with float
 * d2(q, j) != 0 of row_j[b] * w, w = 1.f / d2 (q's own row and those of exact duplicates of q are left
 * out, as in PCL); then each feature's 11 bins are multiplied by 100.f / (their sum) when that sum is not 0.
 * The members are added in the engine's own fixed order (ascending grid position), the feature sums in
 * ascending bin order; FLANN's order is not reproduced.  A keypoint alone in its radius gets 33 zeros, a
 * non-finite keypoint record 33 NaNs.  The same bits in every output on every call.
 * keypoints: record indices in [0, n), in any order, repeats allowed; histogram k belongs to
 * keypoints[k] (NULL: record k, and n_keypoints is ignored).  fpfh: 33 floats at the start of records of
 * fpfh_stride_bytes (>= 132, a multiple of 4), other bytes untouched.
 * MGICP_E_INVALID: a keypoint index outside [0, n), a negative or NaN radius, a bad pointer or stride,
 * a set of more than 65535 records (the rows' uint16 limit; mgicp_last_error names it).  n = 0 or
 * n_keypoints = 0: OK.  float(radius^2) = 0 links nothing: finite keypoints get zeros, every size is 0.
 * Uses the helper cloud slot: a set source / target and their cached state stay as they are.
 * Single rank: with a communicator attached it runs locally, without a collective. */
typedef struct {
    double n_finite;       /* finite records (the searched tree) */
    double n_keypoints;    /* histograms written */
    double n_nan;          /* of those, NaN histograms (non-finite keypoint record) */
    double n_spfh_rows;    /* distinct records whose SPFH row was computed */
    double pair_tests;     /* point-pair distance evaluations the device made */
    double pair_features;  /* computePairFeatures evaluations (self and skipped pairs not counted) */
    double ms_grid;        /* host call -> grid of the finite records built (uploads included) */
    double ms_device;      /* first launch -> stream synchronise after the last */
    double ms_total;       /* host call -> outputs written */
} mgicp_fpfh_info;
int mgicp_fpfh_features(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                        const float* normals, size_t normal_stride_bytes,
                        const int* keypoints /* NULL: every record, in order */, size_t n_keypoints,
                        double radius,
                        float* fpfh, size_t fpfh_stride_bytes /* >= 132, multiple of 4; 132 = pcl::FPFHSignature33 */,
                        uint16_t* spfh_counts /* may be NULL; n * 33 */,
                        int* spfh_sizes /* may be NULL; n */,
                        mgicp_fpfh_info* info /* may be NULL */);

/* InitialAlignment::obtainCorrespondences (src/InitialAlignment.cpp:510-517; every keypoint method calls it
 * on the two feature clouds): pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33>
 * ::determineCorrespondences -- PCL 1.8.1 correspondence_estimation.hpp, KdTreeFLANN with
 * flann::L2_Simple<float> and DefaultPointRepresentation<FPFHSignature33> restated [PCL].  PCL is not
 * available to this project's tests, so parity with PCL binaries is unpinned (README "Parity"); the rules
 * below are the contract, and every deviation from PCL in them is deliberate.
 * Records: 33 floats at the start of records of source_stride_bytes / target_stride_bytes (>= 132, a
 * multiple of 4; 132 = pcl::FPFHSignature33); other bytes are never read as data.
 * Searched set: the target records whose 33 floats are all finite (KdTreeFLANN::convertCloudToArray drops
 * the others and keeps the original indices); match holds original target record indices.
 * Distance: d2(s, t) is a float that starts at 0.0f and takes the bins 0 .. 32 in ascending order, each step
 * diff = s[b] - t[b]; d2 = d2 + diff * diff, without FMA contraction: the product is rounded, then the sum
 * (L2_Simple's loop as x86-64 compiles it).
 * Winner of a source record: among the searched targets with d2 < FLT_MAX (strict: FLANN's result set
 * starts at FLT_MAX) the one with the smallest d2; equal d2 go to the lowest target record index -- the
 * engine's rule; FLANN's choice among equal distances depends on its tree and is not reproduced.
 * Rejection: a source record is dropped when (double)d2 > max_distance * max_distance, in double as PCL
 * evaluates it; DBL_MAX (the reference's call) squares to +inf and rejects nothing.
 * No correspondence (match = -1, distance = NaN): a dropped source record; one with no searched target or
 * with no d2 below FLT_MAX; and, deviation (a), a source record with a non-finite value -- in PCL it trips
 * an assert that release builds compile out and then searches with NaN.
 * distance[i] = the winner's d2 (squared L2, as pcl::Correspondence::distance holds it).
 * *n_correspondences = the matches >= 0; PCL's output is those, in ascending source index.
 * MGICP_E_INVALID: a bad pointer or stride, a negative or NaN max_distance, n_source or n_target above
 * INT32_MAX.  n_source = 0: OK; n_target = 0: OK, every match -1.
 * Exact brute force on the device, split over launches of bounded work (DESIGN.md "Feature
 * correspondences").  The same bits in every output on every call.
 * Uses no cloud slot: a set source / target and their cached state stay as they are.
 * Single rank: with a communicator attached it runs locally, without a collective. */
typedef struct {
    double n_source_valid;    /* source records with 33 finite values */
    double n_target_valid;    /* target records with 33 finite values (the searched set) */
    double n_correspondences; /* source records that got a match */
    double n_tied;            /* matched source records whose minimum is attained by more than one valid target */
    double pair_tests;        /* (source, target) distance evaluations the device began */
    double ms_device;         /* first launch -> stream synchronise after the last */
    double ms_total;          /* host call -> outputs written */
} mgicp_match_info;
int mgicp_match_features(mgicp_ctx* ctx,
                         const float* source, size_t n_source, size_t source_stride_bytes, /* >= 132, multiple of 4 */
                         const float* target, size_t n_target, size_t target_stride_bytes,
                         double max_distance,          /* PCL's argument; DBL_MAX = the reference's call */
                         int* match,                   /* n_source: target record index, -1 = none */
                         float* distance,              /* may be NULL; n_source: squared L2, NaN where match = -1 */
                         size_t* n_correspondences,    /* may be NULL */
                         mgicp_match_info* info        /* may be NULL */);

/* ---- the pre-alignment transform: InitialAlignment::rejectCorrespondences, rejectOneToOneCorrespondences and
 * estimateTransform (src/InitialAlignment.cpp:519-545), the three steps after obtainCorrespondences ----
 * PCL 1.8.1 restated [PCL]: sac.h / ransac.hpp (RandomSampleConsensus::computeModel, SampleConsensus::
 * refineModel), sac_model.h (drawIndexSample, getSamples, computeVariance), sac_model_registration.h(pp),
 * correspondence_rejection_sample_consensus.hpp, correspondence_rejection_one_to_one.cpp,
 * transformation_estimation_svd.hpp and Eigen's umeyama.  PCL is not available to this project's tests, so
 * parity with PCL binaries is unpinned (README "Parity"); the rules below are the contract, and every
 * deviation from PCL in them is named as one.
 * Common to the three calls: a correspondence is (index_query[i], index_match[i], distance[i]), three parallel
 * arrays of length m (pcl::Correspondence's fields).  Keypoint clouds are x, y, z at offsets 0/4/8 of records
 * of the given stride (>= 12, a multiple of 4; 32 = pcl::PointXYZRGB).  MGICP_E_INVALID, before any launch: an
 * index outside its cloud, a bad pointer or stride, m or a cloud size above INT32_MAX.  Plain host pointers; no
 * cloud slot is used: a set source / target, the helper slot and their cached state stay as they are.  The
 * same bits in every output on every call (the info structs' times excepted).  Single rank: with a
 * communicator attached they run locally, without a collective.
 *
 * Model of a set of n pairs (s_k, t_k) -- estimateRigidTransformationSVD of the registration model, umeyama
 * without scaling, in fp64: the 15 sums  sum s (3), sum t (3), sum t_r s_c (9), each term an exact fp64 value;
 * s_mean = sum s / n, t_mean = sum t / n, sigma_rc = (sum t_r s_c) / n - t_mean_r s_mean_c;  sigma = U D V',
 * D descending;  S = diag(1, 1, sign(det U det V));  R = U S V';  t_r = t_mean_r - ((R_r0 s_mean_0 + R_r1
 * s_mean_1) + R_r2 s_mean_2).  The 12 coefficients are rounded to float once (PCL's cast<float>()).
 * Deviation (a): the sums are taken in a fixed tree that depends on n alone -- entry k of the set belongs to
 * lane k % 64 of wave (k / 64) % 4 of block k / 256; a wave adds lanes (l, l + d) for d = 32 .. 1, a block its
 * four waves in order, and block b's sums go to accumulator b % 256, taken in ascending b, the 256 accumulators
 * then through the same wave-and-block tree.  Missing entries are +0.0.  (n = 3: (v0 + v2) + v1.)  PCL demeans
 * first and adds in Eigen's order.  The SVD is a one-sided Jacobi in fp64 inside the library (Eigen uses a
 * two-sided JacobiSVD<Matrix3d>).  A rank-deficient sigma (n < 3, collinear or coincident points) has no
 * unique rotation: the call returns some proper rotation (det +1) and promises no more.
 *
 * Distance of correspondence i under a float model T (rows T_r0 .. T_r3), in float without FMA contraction:
 * p_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 (mgicp_transform_source's formula), d = p - q,
 * d2 = (dx^2 + dz^2) + dy^2 (Eigen's SSE reduction of a 4-vector whose last lane is 0: unpinned, like the
 * rest).  Inlier iff (double)d2 < threshold * threshold, strict, the product in double as PCL takes it. */

/* InitialAlignment::rejectCorrespondences (:519-530): pcl::registration::CorrespondenceRejectorSampleConsensus
 * <PointXYZRGB> with setInlierThreshold(1.5), setRefineModel(true) and its default of 1000 iterations.
 * Sampling (drawIndexSample, getSamples, isSampleGood): an index vector sh starts as the positions 0 .. m-1
 * and is never reset; a draw does, for i = 0, 1, 2, swap(sh[i], sh[i + rnd() % (m - i)]) and takes
 * sh[0 .. 2]; rnd() is boost::uniform_int<>(0, INT_MAX) over boost::mt19937 seeded with 12345: the generator's
 * 32-bit output shifted right by one.  A draw is good iff the three pairwise squared distances of its source
 * points, in float as ((dx^2 + dy^2) + dz^2), all satisfy (double)d > sample_dist_thresh, with
 * sample_dist_thresh = ((sqrt(l0) + sqrt(l1) + sqrt(l2)) / 3)^2 over the singular values l_k (= the
 * eigenvalues, never negative here) of the covariance  sum s s' / m - s_mean s_mean'  of the correspondences'
 * source points.  Up to 1000 draws per sample; if none is good the sample is empty.  Deviation (b): that
 * covariance comes from the fp64 sums of the tree above and the library's Jacobi; PCL computes it in float
 * (computeMeanAndCovarianceMatrix, eigen33).  Deviation (e): PCL shuffles the index_query values and finds a
 * sample's target through a std::map keyed by them; here positions are shuffled, which is the same thing
 * whenever the index_query values are distinct (obtainCorrespondences' output always is).
 * Loop (RandomSampleConsensus::computeModel, probability 0.99): iterations = 0, k = 1, best = -INT_MAX,
 * skipped = 0; while iterations < k and skipped < 10 * max_iterations: take a sample (an empty one ends the
 * loop); its model; count its inliers at `inlier_threshold`; a strictly larger count becomes the best and
 * sets w = best / m, q = min(max(1 - pow(w, 3), DBL_EPSILON), 1 - DBL_EPSILON), k = log(1.0 - 0.99) / log(q);
 * ++iterations; the loop ends when iterations > max_iterations.  (A registration model never fails on three
 * points, so skipped stays 0; max_iterations = 0 therefore runs no iteration.)  The best model's inliers are
 * then selected, ascending.
 * Refine, when `refine` != 0 (SampleConsensus::refineModel(3.0, 1000)): error_threshold = inlier_threshold,
 * prev = the selected inliers, changed = false, rounds = 0; do { the model of prev (an empty prev leaves the
 * model as it is); note |prev|; new = the selection at error_threshold; if new is empty: ++rounds, leave when
 * rounds >= 1000, else go to the loop condition; variance = 2.1981 * the (|new| >> 1)-th smallest (double)d2
 * of new; error_threshold = sqrt(min(inlier_threshold^2, 9 variance)); changed = false; swap(prev, new);
 * if |prev| != |new|: when the last four noted sizes read a, b, a, b the refine ends as "oscillating", else
 * changed = true and go to the loop condition; otherwise changed = (prev != new) } while (changed and
 * ++rounds < 1000).  This is the source's do-while, `continue` jumping to its condition: an empty selection
 * in the first round therefore ends the loop (the issue text read it as "continues"; the source governs).
 * Outcome of the refine: new empty -> failed; oscillating -> succeeded, inliers and model stay those of the
 * loop; not changed -> succeeded, inliers = the selection, model = the last model; else (1000 rounds) failed.
 * Outcomes of the call: keep[i] = 1 for the final inliers (PCL's remaining correspondences are those, in
 * input order), *n_keep their number, best_T_cm the final model (column-major 4 x 4, last row 0 0 0 1).
 * Everything kept (keep all 1, *n_keep = m) and best_T_cm = identity when m < 3, when no model was found
 * (the first sample empty, max_iterations = 0), when the refine failed (PCL logs an error and leaves the
 * caller's vector, which InitialAlignment passes as input and output, untouched), or when fewer than 3 final
 * inliers remain.  MGICP_E_INVALID also for a negative or NaN inlier_threshold and max_iterations < 0.
 * m = 0: OK.  The hypotheses are scored in batches of up to 64 on the device and PCL's sequential loop is
 * replayed over the counts; hypotheses drawn past the loop's end change nothing, since nothing after the
 * loop draws (DESIGN.md "Pre-alignment transform"). */
typedef struct {
    double n_hypotheses;          /* models scored on the device, speculative ones of the last batch included */
    double n_iterations;          /* PCL's iterations_ when its loop ends (0 when m < 3) */
    double n_skipped;             /* PCL's skipped_count (always 0: three points always give a model) */
    double n_refine_rounds;       /* bodies of the refine's do-while that ran */
    double n_inliers_ransac;      /* inliers of the best model at inlier_threshold (0: no model) */
    double n_inliers_final;       /* inliers after the refine (= *n_keep unless everything is kept) */
    double final_error_threshold; /* the refine's error_threshold when it ended (inlier_threshold without one) */
    double pair_tests;            /* pair distance evaluations the device made (scoring and selections) */
    double ms_device;             /* first launch -> stream synchronise after the last, the host's replay,
                                     medians and 3 x 3 solves between them included */
    double ms_total;              /* host call -> outputs written */
} mgicp_ransac_info;
int mgicp_reject_ransac(mgicp_ctx* ctx,
                        const float* source_keypoints, size_t n_source, size_t source_stride_bytes,
                        const float* target_keypoints, size_t n_target, size_t target_stride_bytes,
                        const int* index_query, const int* index_match, size_t m,
                        double inlier_threshold /* the reference: 1.5 */,
                        int max_iterations /* the rejector's default: 1000 */, int refine /* the reference: 1 */,
                        unsigned char* keep /* m */, size_t* n_keep, float best_T_cm[16],
                        mgicp_ransac_info* info /* may be NULL */);

/* InitialAlignment::rejectOneToOneCorrespondences (:532-538): pcl::registration::CorrespondenceRejectorOneToOne.
 * For every index_match value that occurs, the survivor is the correspondence with the smallest distance;
 * deviation (c): equal distances go to the lowest position (PCL's std::sort is unstable there).  order[0 ..
 * *n_keep) = the survivors' positions in ascending index_match, PCL's output order; order[*n_keep .. m) = -1.
 * index_match < 0 is skipped, as in PCL.  MGICP_E_INVALID: index_match >= n_target, a NaN or negative distance
 * (the comparator has no defined answer for NaN), a bad pointer.  -0.0 counts as 0.  m = 0: OK. */
int mgicp_reject_one_to_one(mgicp_ctx* ctx, const int* index_match, const float* distance, size_t m,
                            size_t n_target, int* order /* m */, size_t* n_keep,
                            double* ms_device /* may be NULL: first launch -> stream synchronise */);

/* InitialAlignment::estimateTransform (:540-545): pcl::registration::TransformationEstimationSVD<PointXYZRGB,
 * PointXYZRGB>::estimateRigidTransformation over the correspondences: the model above over all m pairs,
 * T_cm column-major.  Deviation (d): PCL's Scalar is float, so its umeyama runs in float; this call reuses
 * the fp64 path and rounds once.  m = 0: identity.  m of 1 or 2 and rank-deficient sets: the rank rule above. */
typedef struct {
    double sums[15];   /* sum s (3), sum t (3), sum t_r s_c (9, row-major in r), as the tree above gives them */
    double ms_device;  /* first launch -> stream synchronise after the last */
    double ms_total;   /* host call -> output written */
} mgicp_svd_info;
int mgicp_estimate_rigid_svd(mgicp_ctx* ctx,
                             const float* source_keypoints, size_t n_source, size_t source_stride_bytes,
                             const float* target_keypoints, size_t n_target, size_t target_stride_bytes,
                             const int* index_query, const int* index_match, size_t m,
                             float T_cm[16], mgicp_svd_info* info /* may be NULL */);

/* ---- the NORMALS method's own steps: normal clustering and the dominant normals ----
 * InitialAlignment::obtainNormalsCluster (:130-161): pcl::extractEuclideanClusters(cloud, normals, 0.05f, tree,
 * clusters, 20 degrees, 2.5 % of n), the free function's overload with normals, PCL 1.8.1
 * segmentation/extract_clusters.h restated [PCL] (unpinned against PCL binaries, like every feature call).
 * Link: records i != j are linked iff both are finite and FLANN's float ((dx^2 + dy^2) + dz^2) <
 * float(tolerance * tolerance), strict: the predicate of mgicp_euclidean_clusters and mgicp_radius_filter.
 * Compatible with seed s: d = ((n_s.x n_j.x + n_s.y n_j.y) + n_s.z n_j.z) in float without FMA contraction
 * (PCL multiplies floats and widens the sum); j is compatible iff fabs(acos((double)d)) < eps_angle.  PCL
 * compares with the normal of the cluster's SEED (normals.points[i]), not with the normal of the point being
 * expanded.  A NaN d, or d > 1.0f, gives acos = NaN and is not compatible: about 5 % of float-normalised unit
 * vectors have a float self-dot of 1.0000001, and a face whose normals are all bit-identical to such a vector
 * comes out as singletons.  That is PCL's behaviour and is kept.
 * Rounds: `processed` starts false for every finite record; rounds run in ascending s over the unprocessed
 * finite records.  The seed is in its cluster whatever its own normal is.  C_s = the records reachable from s
 * by links through records that were unprocessed at the start of the round and are compatible with s.  All of
 * C_s becomes processed whether or not it is reported: a cluster that is too small still consumes its points,
 * and processed points are never traversed again -- they block the paths of later rounds.  So the result is
 * not a partition by a symmetric predicate: it depends on the seed order and on what earlier rounds consumed.
 * Output: C_s is reported iff max(min_size, 1) <= |C_s| <= max_size (max_size = 0: no cap).  Clusters come in
 * ascending seed (= ascending smallest member; the free function does not sort by size), members ascending.
 * labels / indices / offsets as mgicp_euclidean_clusters.
 * Deviations: (1) non-finite records belong to no round and link to nothing (PCL asserts; the FOD helpers'
 * convention).  (2) PCL skips nn_indices[0] as "the query itself"; with exact duplicates FLANN may put the
 * duplicate first.  Here the link is the predicate above, self excluded, and duplicates link.  (3) libm's acos
 * enters only on the host, once per call: c_min = the smallest float f with acos((double)f) < eps_angle,
 * found by stepping with nextafterf from float(cos(eps_angle)) (20 degrees: 0.9396927f); the device tests
 * d >= c_min && d <= 1.0f.  eps_angle = 0: nothing is compatible; eps_angle > pi: every d in [-1, 1] is.
 * tolerance or eps_angle negative or NaN, bad pointers or strides: MGICP_E_INVALID.  n = 0: no cluster.
 * float(tolerance^2) = 0 links nothing.  The rounds run on the device: small rounds consecutively in one
 * workgroup, a round that outgrows it level by level over the whole device (DESIGN.md "Normal clustering");
 * a round's set is a closure, so neither the split nor the order of claims changes it.
 * Uses the helper cloud slot: a set source / target and their cached state stay as they are.  The same bits
 * in every output on every call (the info struct's times excepted).  Single rank: with a communicator
 * attached it runs locally, without a collective. */
typedef struct {
    double n_rounds;           /* rounds = seeds, singletons and unreported clusters included */
    double n_clusters;         /* reported clusters */
    double n_clustered_points; /* records in reported clusters */
    double n_levels;           /* frontier launches of the level-synchronous path */
    double n_wide_rounds;      /* rounds that left the one-workgroup path */
    double pair_tests;         /* candidate records the expansions walked (each one's processed word is read;
                                  distance and normal are evaluated for the unprocessed ones) */
    double ms_grid;            /* host call -> grid of the finite records built, normals uploaded */
    double ms_device;          /* first launch -> stream synchronise after the member sort, the per-level
                                  read-backs between them included */
    double ms_total;           /* host call -> outputs written */
} mgicp_normal_cluster_info;
int mgicp_normal_clusters(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                          const float* normals /* 3 floats per record */, size_t normal_stride_bytes,
                          double tolerance /* the reference: 0.05f */, double eps_angle /* 20 * (M_PI / 180) */,
                          size_t min_size /* (int)n * 0.025 */, size_t max_size /* 0: no cap */,
                          int* labels /* n */, int* indices /* n */, size_t* offsets /* n + 1 */,
                          mgicp_normal_cluster_info* info /* may be NULL */);

/* InitialAlignment::obtainDominantNormals (:163-187): per cluster c = indices[offsets[c] .. offsets[c + 1]) the
 * sum of the members' normals PLUS THE FIRST MEMBER'S ONCE MORE (the reference starts its accumulator at
 * member 0 and then adds every member), normalised as Eigen's normalize() does: divided by the norm when the
 * squared norm is > 0, else left as it is.  out[3 c ..] = that vector.  A NaN member gives a NaN normal, as in
 * the reference.  Deviation: the sums are fp64, in the fixed tree of the "Model" rule above taken per
 * cluster over its size + 1 entries (entry 0 = the first member, entry 1 + i = member i), which depends on the
 * cluster's size alone; norm = sqrt((x^2 + y^2) + z^2) and the quotients in fp64, rounded to float once.  The
 * reference adds Vector4f's in member order in float.  An empty cluster, an index outside [0, n), bad
 * pointers or strides: MGICP_E_INVALID.  n_clusters = 0: OK.  One segmented launch pair serves every cluster.
 * No cloud slot is used. */
int mgicp_dominant_normals(mgicp_ctx* ctx, const float* normals, size_t n, size_t normal_stride_bytes,
                           const int* indices, const size_t* offsets /* n_clusters + 1 */, size_t n_clusters,
                           float* out /* n_clusters * 3 */,
                           double* ms_device /* may be NULL: first launch -> result on the host */);

/* ---- the FOD-side callers either side of the GICP path ----
 * pcl::SegmentDifferences<PointXYZRGB>::segment as called by Filter::removeFromCloud
 * (src/Filter.cpp:176-189) on the cloud the FSM just transformed with
 * pcl::transformPointCloud (src/LeicaStateMachine.cpp:182; pass that transform as T_cm, or NULL
 * for an already-transformed input).  keep[i] = 1 iff input record i (after T) is finite and
 * its nearest neighbour among the finite points of `sub` has float d^2 > sqr_threshold (PCL's
 * setDistanceThreshold value is compared with the SQUARED distance).  An empty `sub` keeps every
 * record (PCL: output = input).  *n_keep = number of kept records; output order = input order. */
int mgicp_segment_differences(mgicp_ctx* ctx, const float T_cm[16], const float* in, size_t n,
                              size_t in_stride, const float* sub, size_t n_sub, size_t sub_stride,
                              double sqr_threshold, unsigned char* keep, size_t* n_keep);
/* pcl::VoxelGrid<PointXYZRGB>::filter as called by Filter::downsampleCloud (src/Filter.cpp:91-105):
 * one centroid record per occupied leaf (leaf sizes in metres), in ascending leaf index
 * (i + j div_x + k div_x div_y over floor(p / leaf) - floor(min / leaf)).  xyz = fp32 mean
 * (summed in input order), r/g/b/a of the packed colour word at rgb_offset (-1: none) averaged
 * as floats and truncated (CentroidPoint); leaves with fewer than min_points_per_voxel points are
 * dropped; non-finite records skipped.  `out` holds up to n records of out_stride bytes: x, y, z
 * at 0/4/8, 1.0f at 12 (out_stride >= 16), the colour word at rgb_offset, other bytes zero.  When
 * div_x*div_y*div_z exceeds INT32_MAX PCL warns and returns the input: so does this call.
 * rgb_offset is -1 or a multiple of 4 from 12 up that fits both strides; 0, 4 and 8 lie over
 * x, y, z and return MGICP_E_INVALID, as does any other value. */
int mgicp_voxel_grid(mgicp_ctx* ctx, const float* in, size_t n, size_t stride, int rgb_offset,
                     const double leaf[3], int min_points_per_voxel, float* out, size_t out_stride,
                     size_t* n_out);

/* pcl::EuclideanClusterExtraction<PointXYZRGB>::extract as FODDetector::clusterPossibleFODs calls it
 * (src/FODDetector.cpp:45-58) on the difference cloud: the connected components of the graph that
 * links records i != j iff both are finite and FLANN's float d^2 < float(tolerance * tolerance)
 * (strict, as the radius filter above), found by a lock-free union-find over a grid of cell edge
 * tolerance / 2 (DESIGN.md "Euclidean clustering").  A component is a cluster iff
 * max(min_size, 1) <= size <= max_size (max_size = 0: no cap).  Clusters come largest first, equal
 * sizes by ascending smallest member; members ascending.  float(tolerance^2) = 0 links nothing.
 * Non-finite records belong to no cluster.  labels[n]: rank of the record's cluster in output order,
 * -1 none; indices[n]: members, cluster after cluster (the first n_clustered_points entries are
 * written); offsets[n + 1]: cluster c owns indices[offsets[c] .. offsets[c + 1]), entries past the
 * last cluster repeat the total.  tolerance negative or NaN: MGICP_E_INVALID; n = 0: no cluster.
 * Uses the helper cloud slot: a set source / target and their cached state stay as they are.
 * Single rank: with a communicator attached it runs locally, without a collective. */
typedef struct {
    int    n_clusters;         /* reported clusters */
    int    n_components;       /* components of the finite records before the size filter */
    double n_clustered_points; /* records in reported clusters */
    double pair_tests;         /* point-pair distance evaluations the device made */
    double ms_grid;            /* host call -> grid of the finite records built (upload included) */
    double ms_device;          /* host clock from the first launch (forest, links, roots, labels, member
                                  sort; buffers already reserved) to the stream synchronise after the last */
    double ms_total;           /* host call -> outputs written */
} mgicp_cluster_info;
int mgicp_euclidean_clusters(mgicp_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                             double tolerance, size_t min_size, size_t max_size, int* labels,
                             int* indices, size_t* offsets, mgicp_cluster_info* info /* may be NULL */);

/* ---- multi-GPU: one process per GPU, point-range shards of the source cloud ----
 * Rank 0 calls mgicp_get_unique_id and broadcasts the 128 bytes out of band (bench.py uses
 * the TCP rendezvous of leica_point_cloud_processing_amd/parallel.py); every rank then calls
 * mgicp_comm_init before set_* / align.  Every objective pass then all-gathers the ranks' super
 * partials (16 doubles per 32768 source points; GN mode: 80 per super, once per outer iteration)
 * and sums them in a fixed order, so every N gives the single-GPU result bit for bit (see
 * mgicp_debug_supers in mi355x_gicp_debug.h); the target covariances are computed in N slices and all-gathered.  nranks = 1 with an id builds a
 * one-rank communicator (the collective path on a single device); id = NULL makes a "detached"
 * shard for the debug entry points of that header (or an RCCL-free rank, once mgicp_comm_attach_shm succeeds). */
int mgicp_get_unique_id(unsigned char id[128]);
int mgicp_comm_init(mgicp_ctx* ctx, int nranks, int rank, const unsigned char id[128]);
/* Node-local transport of the per-pass sums (all ranks on one node), called by EVERY rank after
 * mgicp_comm_init with the same POSIX shared-memory name ("/..."; unique per job, e.g. chosen by
 * rank 0 and broadcast) and the same max_source_points (0 = 32M; the largest source cloud any
 * later set_source may hold).  It blocks until every rank has mapped the segment, then unlinks the
 * name.  From then on every objective pass writes each rank's super partials straight from its GPU
 * into the segment (resident pass server on every rank, no collective per pass) and every rank's
 * host takes the same fixed-order total; GN moments and fitness gather through it too.  Results
 * stay bitwise those of one GPU.  RCCL (if initialised) is then used only for the one-time
 * all-gather of the target covariances; without it every rank computes them all.  Every rank must
 * run the same sequence of align / fitness calls.  MGICP_E_COMM: segment or peers unavailable (the
 * context keeps its previous transport).  name = NULL detaches (back to RCCL / local). */
int mgicp_comm_attach_shm(mgicp_ctx* ctx, const char* name, size_t max_source_points);
/* r05: per-pass super rows over xGMI instead of host memory (needs mgicp_comm_attach_shm first: the
 * segment carries the IPC rendezvous; every rank calls this in the same sequence).  on = 1: this rank
 * allocates a device exchange buffer, publishes its IPC handle and opens every other rank's; from then
 * on the resident server's super reducers store each row into every rank's buffer (peer device memory,
 * xGMI) and a one-wave totaler per rank takes the fixed-order total on the device -- the host reads one
 * 32-word row per pass instead of every rank's rows.  Sums, iterations and T stay bitwise those of one
 * GPU.  The server leaves one CU to the totaler; a pass that cannot run on the server (another context
 * holds the device's server slot, profiling) returns MGICP_E_COMM.  on = 0 detaches. */
int mgicp_comm_attach_xgmi(mgicp_ctx* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif
