// Stand-alone check of shm::RunningTotal (csrc/shm_rows.hpp) against shm::fixed_total: the total taken
// row by row while the rows land must be fixed_total's, bit for bit, for every super count and for rows
// chosen to expose any change of order or of the starting value.  Prints one "<check> ok|FAIL" line per
// check and the time of one total over 153 rows in both forms.  Exit status 1 on any FAIL.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "shm_rows.hpp"

using mgicp::shm::fixed_total;
using mgicp::shm::RunningTotal;

namespace {

constexpr int kNv = 16;
const long long kSups[] = {1, 2, 63, 64, 65, 127, 128, 129, 153, 192, 193};

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
double unit() { return static_cast<double>(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

// row generators: value v of super s
double gen_uniform(long long, int) { return unit() - 0.5; }
// magnitudes 1e-300 ... 1e300 mixed within one lane (supers s, s + 64, s + 128 share a lane)
double gen_magnitudes(long long s, int v) {
  static const double mags[] = {1e-300, 1e300, 1e-150, 1.0, 1e150, 1e-30, 1e30};
  const double m = mags[(s / 64 + s + v) % 7];
  return (unit() - 0.5) * m;
}
// cancelling pairs: super s + 64 is the negative of super s, so a lane's partial passes through 0
double g_pair[256][kNv];
double gen_cancel(long long s, int v) {
  if ((s / 64) & 1) return -g_pair[s - 64][v];
  g_pair[s][v] = (unit() - 0.5) * 1e12;
  return g_pair[s][v];
}
double gen_neg_zero(long long, int) { return -0.0; }
// -0.0 first rows, then a mix of zeros of both signs and values
double gen_zero_mix(long long s, int) {
  if (s < 64) return -0.0;
  const uint64_t k = next_u64() % 4;
  return k == 0 ? -0.0 : (k == 1 ? 0.0 : (k == 2 ? unit() : -unit()));
}
double gen_denormal(long long s, int v) {
  const double d = std::numeric_limits<double>::denorm_min() * static_cast<double>(1 + next_u64() % 1000);
  return ((s + v) & 1) ? -d : d;
}
// denormals beside normals whose sum falls back into the denormal range
double gen_denormal_mix(long long s, int) {
  const double tiny = std::numeric_limits<double>::min();
  const uint64_t k = next_u64() % 3;
  return k == 0 ? tiny * unit() : (k == 1 ? -tiny * unit() : tiny * (unit() - 0.5) * 4.0) * ((s & 1) ? 1.0 : -1.0);
}

struct Gen {
  const char* name;
  double (*fn)(long long, int);
};
const Gen kGens[] = {{"uniform", gen_uniform},       {"magnitudes", gen_magnitudes}, {"cancelling_pairs", gen_cancel},
                     {"negative_zero_rows", gen_neg_zero}, {"zero_sign_mix", gen_zero_mix}, {"denormals", gen_denormal},
                     {"denormal_mix", gen_denormal_mix}};

bool same_total(const std::vector<double>& rows, long long nsup) {
  double want[kNv], got[kNv];
  fixed_total(rows.data(), nsup, kNv, want);
  RunningTotal rt;
  rt.reset();
  for (long long r = 0; r < nsup; ++r) rt.add_row(r, rows.data() + static_cast<size_t>(r) * kNv);
  rt.finish(got);
  return std::memcmp(want, got, sizeof(want)) == 0;
}

double median_ns(std::vector<double>& t) {
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}

}  // namespace

int main() {
  bool all = true;
  for (const Gen& g : kGens) {
    bool ok = true;
    for (int rep = 0; rep < 50; ++rep)
      for (long long nsup : kSups) {
        std::vector<double> rows(static_cast<size_t>(nsup) * kNv);
        for (long long s = 0; s < nsup; ++s)
          for (int v = 0; v < kNv; ++v) rows[static_cast<size_t>(s) * kNv + v] = g.fn(s, v);
        if (!same_total(rows, nsup)) {
          ok = false;
          std::printf("# %s: nsup %lld differs\n", g.name, nsup);
        }
      }
    std::printf("%s %s\n", g.name, ok ? "ok" : "FAIL");
    all = all && ok;
  }
  {  // a -0.0 only total is +0.0 in both forms (the lanes start from +0.0), for one row and for many
    bool ok = true;
    for (long long nsup : kSups) {
      std::vector<double> rows(static_cast<size_t>(nsup) * kNv, -0.0);
      double got[kNv];
      RunningTotal rt;
      rt.reset();
      for (long long r = 0; r < nsup; ++r) rt.add_row(r, rows.data() + static_cast<size_t>(r) * kNv);
      rt.finish(got);
      for (int v = 0; v < kNv; ++v) ok = ok && got[v] == 0.0 && !std::signbit(got[v]);
      ok = ok && same_total(rows, nsup);
    }
    std::printf("negative_zero_total_is_positive %s\n", ok ? "ok" : "FAIL");
    all = all && ok;
  }
  {  // a RunningTotal reused after reset() gives the same total again
    std::vector<double> rows(153 * kNv);
    for (double& x : rows) x = gen_magnitudes(next_u64() % 153, 0);
    double a[kNv], b[kNv];
    RunningTotal rt;
    for (double* out : {a, b}) {
      rt.reset();
      for (long long r = 0; r < 153; ++r) rt.add_row(r, rows.data() + static_cast<size_t>(r) * kNv);
      rt.finish(out);
    }
    const bool ok = std::memcmp(a, b, sizeof(a)) == 0 && same_total(rows, 153);
    std::printf("reuse_after_reset %s\n", ok ? "ok" : "FAIL");
    all = all && ok;
  }
  {  // the time of one total over 153 rows (C4's super count): what is left after the last row lands is
     // the whole of fixed_total in the old form and finish() alone in the new one
    constexpr int kReps = 10000;
    const long long nsup = 153;
    std::vector<double> rows(static_cast<size_t>(nsup) * kNv);
    for (double& x : rows) x = unit() - 0.5;
    std::vector<double> t_old(kReps), t_new(kReps), t_all(kReps);
    double sink = 0.0, out[kNv];
    for (int i = 0; i < kReps; ++i) {
      rows[static_cast<size_t>(i % nsup) * kNv] = unit();
      auto a = std::chrono::steady_clock::now();
      fixed_total(rows.data(), nsup, kNv, out);
      auto b = std::chrono::steady_clock::now();
      sink += out[0];
      t_old[i] = std::chrono::duration<double, std::nano>(b - a).count();
      RunningTotal rt;
      auto c = std::chrono::steady_clock::now();
      rt.reset();
      for (long long r = 0; r < nsup; ++r) rt.add_row(r, rows.data() + static_cast<size_t>(r) * kNv);
      auto d = std::chrono::steady_clock::now();
      rt.finish(out);
      auto e = std::chrono::steady_clock::now();
      sink += out[0];
      t_new[i] = std::chrono::duration<double, std::nano>(e - d).count();
      t_all[i] = std::chrono::duration<double, std::nano>(e - c).count();
    }
    std::printf("# time of one total, 153 rows x 16 values, median of %d: fixed_total %.0f ns | RunningTotal after the "
                "last row (finish) %.0f ns, reset + 153 add_row + finish %.0f ns (sink %g)\n",
                kReps, median_ns(t_old), median_ns(t_new), median_ns(t_all), sink);
  }
  return all ? 0 : 1;
}
