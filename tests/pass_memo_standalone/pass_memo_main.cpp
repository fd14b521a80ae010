// Stand-alone check of csrc/pass_memo.hpp under csrc/pcl_bfgs.hpp (no HIP, no device): tests/test_pass_memo.py
// builds it with g++, plain and with -fsanitize=address,undefined, and reads the lines it prints.
//
// StubFunctor has the device functor's structure (DeviceFunctor, mgicp_pass.hip): a "pass" sees the BFGS
// state x only through an fp32 3x4 transform A(x) and returns 16 raw sums over a few hundred synthetic
// correspondences; f and g come from those sums and the doubles of x on the "host"; the last x is
// memoised; with the table on, a new x whose A the run has passed over already takes the held sums.
// PclBfgs runs over it as estimate_bfgs runs it (first pass seeds memo and table, init, steps until the
// line search makes no progress), once with the table and once without, and every (x, f, g) the solver
// was handed is compared bitwise.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pass_memo.hpp"
#include "pcl_bfgs.hpp"

using mgicp::PassMemo;
using mgicp::PclBfgs;
using mgicp::Vec6;

namespace {

int g_failed = 0;
void check(const char* name, bool ok) {
  std::printf("%s %s\n", name, ok ? "ok" : "FAIL");
  if (!ok) ++g_failed;
}

// R = Rz(x5) Ry(x4) Rx(x3) from elementary rotations; which = 0 / 1 / 2 replaces Rx / Ry / Rz by its derivative
template <class T>
void rot(T phi, T theta, T psi, int which, T R[3][3]) {
  const T a[3] = {phi, theta, psi};
  T E[3][3][3];
  for (int k = 0; k < 3; ++k) {
    const T c = std::cos(a[k]), s = std::sin(a[k]);
    const bool d = which == k;
    const T cc = d ? -s : c, ss = d ? c : s, one = d ? T(0) : T(1);
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    for (int u = 0; u < 3; ++u)
      for (int v = 0; v < 3; ++v) E[k][u][v] = T(0);
    E[k][k][k] = one;
    E[k][i][i] = cc;
    E[k][j][j] = cc;
    E[k][i][j] = -ss;
    E[k][j][i] = ss;
  }
  T M[3][3];
  for (int u = 0; u < 3; ++u)
    for (int v = 0; v < 3; ++v) {
      M[u][v] = T(0);
      for (int w = 0; w < 3; ++w) M[u][v] += E[1][u][w] * E[0][w][v];
    }
  for (int u = 0; u < 3; ++u)
    for (int v = 0; v < 3; ++v) {
      R[u][v] = T(0);
      for (int w = 0; w < 3; ++w) R[u][v] += E[2][u][w] * M[w][v];
    }
}

// the fp32 transform of a state: all a pass sees of x
void transform_of(const Vec6& x, float A[12]) {
  float R[3][3];
  rot<float>(static_cast<float>(x[3]), static_cast<float>(x[4]), static_cast<float>(x[5]), -1, R);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) A[4 * i + j] = R[i][j];
    A[4 * i + 3] = 0.0f + static_cast<float>(x[i]);
  }
}

struct Eval {
  Vec6 x;
  double f;
  Vec6 g;
};

struct StubFunctor {
  explicit StubFunctor(bool table) : use_table(table) {}
  bool use_table;
  std::vector<float> p, q;  // correspondences: 3 floats each
  bool have_memo = false;
  Vec6 memo_x{};
  double memo_f = 0;
  Vec6 memo_g{};
  PassMemo seen{};
  long passes = 0, hits = 0;
  std::vector<Eval> log;  // every evaluation handed to the solver

  // the "device": residuals through the fp32 A only; fixed order, so the sums are a function of A
  void pass(const Vec6& x, double s[16]) {
    float A[12];
    transform_of(x, A);
    for (int i = 0; i < 16; ++i) s[i] = 0.0;
    const size_t n = p.size() / 3;
    for (size_t k = 0; k < n; ++k) {
      const float* a = &p[3 * k];
      const float* b = &q[3 * k];
      double r[3];
      for (int i = 0; i < 3; ++i) {
        const float y = ((A[4 * i] * a[0] + A[4 * i + 1] * a[1]) + A[4 * i + 2] * a[2]) + A[4 * i + 3];
        r[i] = static_cast<double>(y) - static_cast<double>(b[i]);
      }
      // Mahalanobis matrix I / epsilon, GICP's epsilon 0.001: the scale at which its gradient tolerance
      // 1e-2 lies below what fp32 A resolves, so a run ends in the line search, as the engine's runs do
      const double w = 1000.0;
      s[0] += w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      for (int i = 0; i < 3; ++i) {
        s[1 + i] += w * r[i];
        for (int j = 0; j < 3; ++j) s[4 + 3 * i + j] += w * r[i] * static_cast<double>(a[j]);
      }
      s[13] += 1.0;
    }
    ++passes;
  }
  // the "host": f and g at x from the sums of the pass at x (g's rotation part reads the doubles of x)
  void memoise(const Vec6& x, const double s[16]) {
    const double m = s[13], sc = 2.0 / m;
    memo_x = x;
    memo_f = s[0] / m;
    for (int i = 0; i < 3; ++i) memo_g[i] = s[1 + i] * sc;
    for (int a = 0; a < 3; ++a) {
      double dR[3][3], r = 0.0;
      rot<double>(x[3], x[4], x[5], a, dR);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r += dR[i][j] * s[4 + 3 * i + j] * sc;
      memo_g[3 + a] = r;
    }
    have_memo = true;
  }
  void remember(const Vec6& x, const double s[16]) {
    float A[12];
    transform_of(x, A);
    if (use_table) seen.insert(A, s);
  }
  int eval(const Vec6& x, double& f, Vec6& g) {
    if (!(have_memo && std::memcmp(x.v, memo_x.v, sizeof(x.v)) == 0)) {
      float A[12];
      transform_of(x, A);
      const double* held = use_table ? seen.find(A) : nullptr;
      if (held) {
        ++hits;
        memoise(x, held);
      } else {
        double s[16];
        pass(x, s);
        if (use_table) seen.insert(A, s);
        memoise(x, s);
      }
    }
    f = memo_f;
    g = memo_g;
    log.push_back({x, f, g});
    return 0;
  }
};

// a scan of a box-like part against itself moved by a small rigid motion, plus noise the motion cannot
// explain: the minimum has a residual, and near it fp32 A stops resolving the line search's steps
void make_pairs(unsigned seed, int n, std::vector<float>& p, std::vector<float>& q) {
  uint32_t st = seed;
  auto rnd = [&st]() {  // uniform in [0, 1)
    st = st * 1664525u + 1013904223u;
    return static_cast<float>(st >> 8) * (1.0f / 16777216.0f);
  };
  Vec6 xt{{1.3, -2.1, 0.8, 0.02, -0.015, 0.03}};
  float A[12];
  transform_of(xt, A);
  p.resize(3 * static_cast<size_t>(n));
  q.resize(3 * static_cast<size_t>(n));
  for (int k = 0; k < n; ++k) {
    float* a = &p[3 * k];
    a[0] = 6.0f * rnd() - 3.0f;
    a[1] = 4.0f * rnd() - 2.0f;
    a[2] = 2.0f * rnd() - 1.0f;
    for (int i = 0; i < 3; ++i)
      q[3 * k + i] = A[4 * i] * a[0] + A[4 * i + 1] * a[1] + A[4 * i + 2] * a[2] + A[4 * i + 3] + 0.002f * (rnd() - 0.5f);
  }
}

struct RunResult {
  Vec6 x;
  long passes, hits;
  std::vector<Eval> log;
};

// GICP::estimateRigidTransformationBFGS as estimate_bfgs (mgicp_engine.hip) runs it, over the stub
RunResult run(bool use_table, unsigned seed, const Vec6& x0, int max_inner) {
  StubFunctor fn(use_table);
  make_pairs(seed, 300, fn.p, fn.q);
  Vec6 x = x0;
  double s[16];
  fn.pass(x, s);
  fn.memoise(x, s);
  fn.remember(x, s);
  PclBfgs<StubFunctor> bfgs(fn);
  int inner = 0;
  int result = bfgs.init(x);
  result = mgicp::kRunning;
  do {
    inner++;
    result = bfgs.step(x);
    if (result) break;
    result = bfgs.test_gradient(1e-2);
  } while (result == mgicp::kRunning && inner < max_inner);
  return RunResult{x, fn.passes, fn.hits, fn.log};
}

bool same_log(const std::vector<Eval>& a, const std::vector<Eval>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (std::memcmp(a[i].x.v, b[i].x.v, sizeof(a[i].x.v)) != 0 || std::memcmp(&a[i].f, &b[i].f, sizeof(double)) != 0 ||
        std::memcmp(a[i].g.v, b[i].g.v, sizeof(a[i].g.v)) != 0)
      return false;
  return true;
}

void solver_checks() {
  // four runs as the outer iterations of an align chain them: each starts where the last one ended, over
  // other correspondences, with a table of its own
  Vec6 x0{{0, 0, 0, 0, 0, 0}};
  long passes_on = 0, passes_off = 0, hits_on = 0, hits_off = 0;
  bool logs = true, finals = true;
  size_t evals = 0;
  for (unsigned r = 0; r < 4; ++r) {
    const RunResult off = run(false, 17u + r, x0, 200);
    const RunResult on = run(true, 17u + r, x0, 200);
    std::printf("run %u evaluations %zu passes_without %ld passes_with %ld hits %ld\n", r, off.log.size(), off.passes,
                on.passes, on.hits);
    logs = logs && same_log(on.log, off.log);
    finals = finals && std::memcmp(on.x.v, off.x.v, sizeof(on.x.v)) == 0;
    passes_on += on.passes;
    passes_off += off.passes;
    hits_on += on.hits;
    hits_off += off.hits;
    evals += off.log.size();
    x0 = off.x;
  }
  std::printf("total evaluations %zu passes_without %ld passes_with %ld hits %ld\n", evals, passes_off, passes_on, hits_on);
  check("solver_evaluations_bitwise_equal", logs);
  check("solver_final_x_bitwise_equal", finals);
  check("solver_fewer_passes_with_table", passes_on < passes_off && hits_on > 0);
  check("solver_hits_plus_passes_equal_untabled_passes", hits_on + passes_on == passes_off);
  check("solver_no_hits_without_table", hits_off == 0);
}

void table_checks() {
  static PassMemo t;  // ~45 KB: not on this frame beside the runs'
  float key[12];
  double sums[16];
  auto fill = [&](int i) {
    for (int k = 0; k < 12; ++k) key[k] = static_cast<float>(i) + 0.25f * static_cast<float>(k);
    for (int k = 0; k < 16; ++k) sums[k] = 1000.0 * i + k;
  };
  bool ok = true;
  for (int i = 0; i < PassMemo::kCap; ++i) {
    fill(i);
    ok = ok && t.find(key) == nullptr && t.insert(key, sums);
  }
  check("table_fills_to_capacity", ok && t.n == PassMemo::kCap);
  fill(PassMemo::kCap);
  check("table_full_stops_inserting", !t.insert(key, sums) && t.n == PassMemo::kCap && t.find(key) == nullptr);
  ok = true;
  for (int i = 0; i < PassMemo::kCap; ++i) {
    fill(i);
    const double* s = t.find(key);
    ok = ok && s && std::memcmp(s, sums, sizeof(sums)) == 0;
  }
  check("table_full_keeps_every_entry", ok);

  static PassMemo z;
  fill(3);
  key[7] = 0.0f;
  double plus[16], minus[16];
  for (int k = 0; k < 16; ++k) plus[k] = 1.0 + k, minus[k] = -1.0 - k;
  z.insert(key, plus);
  key[7] = -0.0f;
  check("table_zero_sign_is_a_miss", z.find(key) == nullptr);
  z.insert(key, minus);
  const double* sm = z.find(key);
  key[7] = 0.0f;
  const double* sp = z.find(key);
  check("table_zero_signs_are_two_keys",
        z.n == 2 && sm && sp && std::memcmp(sm, minus, sizeof(minus)) == 0 && std::memcmp(sp, plus, sizeof(plus)) == 0);

  static PassMemo f;
  const float bad[3] = {std::nanf(""), INFINITY, -INFINITY};
  ok = true;
  for (int b = 0; b < 3; ++b)
    for (int k = 0; k < 12; ++k) {
      fill(5);
      key[k] = bad[b];
      ok = ok && !PassMemo::finite(key) && !f.insert(key, sums) && f.n == 0 && f.find(key) == nullptr;
    }
  check("table_refuses_non_finite_keys", ok);
  fill(5);
  check("table_takes_the_finite_key", PassMemo::finite(key) && f.insert(key, sums) && f.n == 1 && f.find(key) != nullptr);
  // a NaN key equal bit for bit to nothing stored must not match by accident, nor a stored key match a NaN one
  key[0] = bad[0];
  check("table_non_finite_lookup_misses", f.find(key) == nullptr);
}

}  // namespace

int main() {
  table_checks();
  solver_checks();
  std::printf("failed %d\n", g_failed);
  return g_failed ? 1 : 0;
}
