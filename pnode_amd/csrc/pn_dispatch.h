// pnode_amd -- host-side dispatch helpers shared by every kernel file: the 16-byte alignment test, the grid size of a
// launch, and the three steps from a run-time value (operand count, dtype, vector or scalar form) to the template argument
// of a kernel.  Pure C++17, no HIP include: also read by plain g++ (tests/native/dispatch_check.cpp).
//
// The callables receive a tag (std::integral_constant<int, N>, or a value of the element type) and are called directly:
// no std::function, no allocation, no virtual call -- these sit on the path of every launch.
#pragma once
#include <cstdint>
#include <type_traits>
#include <utility>

#include "pnode_amd.h"

namespace pn {

// a null pointer counts as aligned: an absent optional operand never forces the scalar form
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <typename... P>
inline bool aligned16(const void *p, const P *...more) {
  return aligned16(p) && aligned16(more...);
}
// every entry of a pointer table
inline bool aligned16(const void *const *p, int count) {
  for (int j = 0; j < count; ++j)
    if (!aligned16(p[j])) return false;
  return true;
}

// workgroups for `items` at `per_block` each: rounded up, at least 1, at most `cap` where cap > 0
inline int64_t blocks_for(int64_t items, int64_t per_block, int64_t cap = 0) {
  const int64_t nb = (items + per_block - 1) / per_block;
  if (nb < 1) return 1;
  return cap > 0 && nb > cap ? cap : nb;
}

// what with_count / with_dtype return when they have no case for the value: the caller turns it into its own refusal
constexpr int kNoCase = -1;

template <int LO, typename F, int... I>
inline int with_count_seq(int n, F &f, std::integer_sequence<int, I...>) {
  int rc = kNoCase;
  (void)((n == LO + I ? (rc = f(std::integral_constant<int, LO + I>{}), true) : false) || ...);
  return rc;
}
// f(integral_constant<int, N>{}) for the N == n of [LO, HI]; f is instantiated for exactly LO..HI
template <int LO, int HI, typename F>
inline int with_count(int n, F &&f) {
  static_assert(LO <= HI, "empty range");
  return with_count_seq<LO>(n, f, std::make_integer_sequence<int, HI - LO + 1>{});
}

// f(float{}) for PN_F32, f(double{}) for PN_F64
template <typename F>
inline int with_dtype(int dtype, F &&f) {
  if (dtype == PN_F32) return f(float{});
  if (dtype == PN_F64) return f(double{});
  return kNoCase;
}

// the vector form (16 bytes of T per access) or the scalar form of the same kernel
template <typename T, typename F>
inline int with_width(bool vec, F &&f) {
  return vec ? f(std::integral_constant<int, (int)(16 / sizeof(T))>{}) : f(std::integral_constant<int, 1>{});
}

}  // namespace pn
