// Host checks of an entry point's pointer arguments.  (Not in common.hpp:
// the GEMM tuning database is stamped with a digest that covers that file.)
#pragma once
#include <cstddef>
#include <cstdint>

namespace s3 {

// p is a-byte aligned (a: a power of two)
inline bool aligned(const void* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

// the byte ranges [a, a + na) and [b, b + nb) intersect
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

}  // namespace s3
