// prealign.hpp -- the host arithmetic of the pre-alignment transform (include/mi355x_gicp.h "the
// pre-alignment transform"): the 3 x 3 fp64 Jacobi SVD, the model of a point set from its 15 sums, the
// sample-distance threshold, the strict float form of the inlier test and PCL's sample stream.  Plain C++,
// no HIP: mgicp_features.hip drives the kernels with it.  Include it from a file compiled without FMA
// contraction.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <random>
#include <vector>

namespace mgicp {
namespace prealign {

inline double det3(const double M[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// A = U diag(D) V' (all row-major), D descending, U and V orthogonal.  One-sided (Hestenes) Jacobi: the
// columns of A are rotated against each other until they are orthogonal to rounding; their norms are D,
// the normalised columns U, the accumulated rotations V.  Columns of norm 0 get U columns that complete an
// orthonormal basis (rank 2: the cross product of the other two).
inline void svd3(const double A[9], double U[9], double D[3], double V[9]) {
  double w[3][3], v[3][3];  // [column][row]
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) {
      w[c][r] = A[3 * r + c];
      v[c][r] = r == c ? 1.0 : 0.0;
    }
  auto dot = [](const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
  static const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (const auto& pq : pairs) {
      double* wp = w[pq[0]];
      double* wq = w[pq[1]];
      const double a = dot(wp, wp), b = dot(wq, wq), g = dot(wp, wq);
      if (g == 0.0 || std::fabs(g) <= std::numeric_limits<double>::epsilon() * std::sqrt(a) * std::sqrt(b)) continue;
      rotated = true;
      const double zeta = (b - a) / (2.0 * g);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
      const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
      double* vp = v[pq[0]];
      double* vq = v[pq[1]];
      for (int r = 0; r < 3; ++r) {
        const double x = wp[r], y = wq[r];
        wp[r] = cs * x - sn * y;
        wq[r] = sn * x + cs * y;
        const double vx = vp[r], vy = vq[r];
        vp[r] = cs * vx - sn * vy;
        vq[r] = sn * vx + cs * vy;
      }
    }
    if (!rotated) break;
  }
  double nrm[3];
  int ord[3] = {0, 1, 2};
  for (int c = 0; c < 3; ++c) nrm[c] = std::sqrt(dot(w[c], w[c]));
  std::stable_sort(ord, ord + 3, [&](int x, int y) { return nrm[x] > nrm[y]; });
  double u[3][3];
  int rank = 0;
  for (int k = 0; k < 3; ++k) {
    const int c = ord[k];
    D[k] = nrm[c];
    for (int r = 0; r < 3; ++r) V[3 * r + k] = v[c][r];
    if (nrm[c] > 0.0 && std::isfinite(nrm[c])) {
      for (int r = 0; r < 3; ++r) u[k][r] = w[c][r] / nrm[c];
      rank = k + 1;
    }
  }
  auto cross = [](const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  if (rank == 0) {
    for (int k = 0; k < 3; ++k)
      for (int r = 0; r < 3; ++r) u[k][r] = r == k ? 1.0 : 0.0;
  } else if (rank == 1) {
    int e = 0;  // the axis least along u0
    for (int r = 1; r < 3; ++r)
      if (std::fabs(u[0][r]) < std::fabs(u[0][e])) e = r;
    double x[3] = {0.0, 0.0, 0.0};
    x[e] = 1.0;
    const double p = u[0][e];
    for (int r = 0; r < 3; ++r) x[r] -= p * u[0][r];
    const double n = std::sqrt(dot(x, x));
    for (int r = 0; r < 3; ++r) u[1][r] = x[r] / n;
    cross(u[0], u[1], u[2]);
  } else if (rank == 2) {
    cross(u[0], u[1], u[2]);
  }
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) U[3 * r + k] = u[k][r];
}

// the model of n pairs from their 15 sums (sum s, sum t, sum t_r s_c): the rows of a 3 x 4, rounded to float
inline void model_from_sums(const double sums[15], double n, float T[12]) {
  double sm[3], tm[3], sigma[9];
  for (int r = 0; r < 3; ++r) sm[r] = sums[r] / n, tm[r] = sums[3 + r] / n;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sigma[3 * r + c] = sums[6 + 3 * r + c] / n - tm[r] * sm[c];
  double U[9], D[3], V[9];
  svd3(sigma, U, D, V);
  const double s2 = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
  for (int r = 0; r < 3; ++r) {
    double R[3];
    for (int c = 0; c < 3; ++c) R[c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + s2 * U[3 * r + 2] * V[3 * c + 2];
    const double t = tm[r] - ((R[0] * sm[0] + R[1] * sm[1]) + R[2] * sm[2]);
    for (int c = 0; c < 3; ++c) T[4 * r + c] = static_cast<float>(R[c]);
    T[4 * r + 3] = static_cast<float>(t);
  }
}

// sample_dist_thresh from the 15 sums of the source points paired with themselves (sums[6..] = sum s s')
inline double sample_dist_thresh(const double sums[15], double n) {
  double sm[3], cov[9];
  for (int r = 0; r < 3; ++r) sm[r] = sums[r] / n;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) cov[3 * r + c] = sums[6 + 3 * r + c] / n - sm[r] * sm[c];
  double U[9], D[3], V[9];
  svd3(cov, U, D, V);
  const double t = ((std::sqrt(D[0]) + std::sqrt(D[1])) + std::sqrt(D[2])) / 3.0;
  return t * t;
}

// the float lim with  d2 < lim  <=>  (double)d2 < thr2  for every float d2: the smallest float whose
// double value is not below thr2 (thr2 >= 0, not NaN; +inf when thr2 is above every float)
inline float strict_limit(double thr2) {
  float f = static_cast<float>(thr2);
  if (static_cast<double>(f) < thr2) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
  return f;
}

// the 15 sums of three pairs in the tree's order for n = 3: (v0 + v2) + v1, then + 0.0 as the upper levels add
inline void sums_of_three(const float s[3][3], const float t[3][3], double sums[15]) {
  auto tree = [](double a, double b, double c) { return ((a + c) + b) + 0.0; };
  for (int r = 0; r < 3; ++r) {
    sums[r] = tree(s[0][r], s[1][r], s[2][r]);
    sums[3 + r] = tree(t[0][r], t[1][r], t[2][r]);
    for (int c = 0; c < 3; ++c)
      sums[6 + 3 * r + c] = tree(static_cast<double>(t[0][r]) * s[0][c], static_cast<double>(t[1][r]) * s[1][c],
                                 static_cast<double>(t[2][r]) * s[2][c]);
  }
}

// PCL's sample stream over m positions (drawIndexSample, getSamples, isSampleGood)
struct Sampler {
  std::mt19937 gen{12345u};  // boost::mt19937's parameters and seeding
  std::vector<int> sh;
  explicit Sampler(size_t m) : sh(m) {
    for (size_t i = 0; i < m; ++i) sh[i] = static_cast<int>(i);
  }
  // uniform_int<>(0, INT_MAX) over a 32-bit engine: two engine values per bucket
  uint32_t rnd() { return static_cast<uint32_t>(gen()) >> 1; }
  void draw(int out[3]) {
    const size_t m = sh.size();
    for (size_t i = 0; i < 3; ++i) std::swap(sh[i], sh[i + rnd() % (m - i)]);
    out[0] = sh[0], out[1] = sh[1], out[2] = sh[2];
  }
  static bool far(const float* a, const float* b, double thresh) {
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const float d = (dx * dx + dy * dy) + dz * dz;
    return static_cast<double>(d) > thresh;
  }
  // a good sample within 1000 draws, or false; sxyz: packed source points, iq: each position's source record
  bool sample(const float* sxyz, const int* iq, double thresh, int out[3]) {
    if (sh.size() < 3) return false;
    for (int it = 0; it < 1000; ++it) {
      draw(out);
      const float* p0 = sxyz + 3 * static_cast<size_t>(iq[out[0]]);
      const float* p1 = sxyz + 3 * static_cast<size_t>(iq[out[1]]);
      const float* p2 = sxyz + 3 * static_cast<size_t>(iq[out[2]]);
      if (far(p0, p1, thresh) && far(p0, p2, thresh) && far(p1, p2, thresh)) return true;
    }
    return false;
  }
};

}  // namespace prealign
}  // namespace mgicp
