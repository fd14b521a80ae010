// pass_memo.hpp -- the objective passes a BFGS run has already paid for, keyed on what the device saw.
//
// An objective pass depends on the BFGS state x (6 doubles) only through the fp32 3x4 transform
// A = apply_state(x): the kernels never see x, and their 16 raw sums are bitwise a function of A and
// the run's correspondences (same chunks, lane order and tree on every pass path, in either sweep
// direction, on any rank count).  PCL's line search ends most runs by shrinking alpha below what fp32
// can express in A, and then keeps asking for f at states whose doubles differ but whose A is
// bit-identical to one already evaluated in the run (DESIGN.md "Redundant passes").  This table holds
// (A, sums) of the run's passes so that such a request costs a look-up instead of a device pass; the
// caller turns the stored sums into f and g with the NEW x, exactly as it would the sums of a pass.
//
// One table per BFGS run: the sums belong to the run's correspondences, and the first A of the next
// run is normally the last A of this one, over other correspondences.  Pure C++ (no HIP), so the
// solver and the table can be compiled and tested on their own.
#pragma once
#include <cstdint>
#include <cstring>

namespace mgicp {

struct PassMemo {
  static constexpr int kKeyFloats = 12;  // Xf34: the 3x4 transform, row-major
  static constexpr int kVals = 16;       // kRedVals: the raw sums of one pass
  // a run has at most a few hundred evaluations (max_inner_iter steps of a line search that mostly ends
  // within ten); a full table stops inserting, which is exact: a miss is a pass
  static constexpr int kCap = 256;

  struct Entry {
    float key[kKeyFloats];
    double sums[kVals];
  };
  Entry e[kCap];
  int n = 0;

  // Inf or NaN in any word: such a key is neither stored nor looked up (a NaN has many bit patterns,
  // and a state that far gone should fail the way it always has, through a pass)
  static bool finite(const float* A) {
    for (int i = 0; i < kKeyFloats; ++i) {
      uint32_t w;
      std::memcpy(&w, A + i, sizeof(w));
      if ((w & 0x7f800000u) == 0x7f800000u) return false;
    }
    return true;
  }

  // the sums stored under the 48 bytes of A, or nullptr.  Bitwise: +0.0f and -0.0f are different keys
  // (a kernel may tell them apart, the table must not have to know).  Newest first: a repeat is
  // nearly always the pass before.
  const double* find(const float* A) const {
    if (!finite(A)) return nullptr;
    for (int i = n - 1; i >= 0; --i)
      if (std::memcmp(e[i].key, A, sizeof(e[i].key)) == 0) return e[i].sums;
    return nullptr;
  }

  // false: not stored (table full, or a non-finite key)
  bool insert(const float* A, const double* s) {
    if (n >= kCap || !finite(A)) return false;
    std::memcpy(e[n].key, A, sizeof(e[n].key));
    std::memcpy(e[n].sums, s, sizeof(e[n].sums));
    ++n;
    return true;
  }
};

}  // namespace mgicp
