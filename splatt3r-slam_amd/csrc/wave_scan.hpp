// Wave (64 lanes) and workgroup scans of one uint32 per thread, and the wave
// primitives of the radix pass (radix_pass.hpp).  Device-only; every kernel
// file that compacts or sorts includes this and keeps no copy of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace s3 {

__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v = max(v, t);
  }
  return v;
}

// Exclusive sum of one value per thread across a workgroup of NT threads
// (every thread calls it); *total receives the workgroup's sum.  s_w: NT / 64
// words of LDS.  One barrier after the wave partials are written and one
// after they are read, so back-to-back calls may share s_w.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_add(uint32_t v, uint32_t* s_w,
                                                   uint32_t* total = nullptr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_add(v, lane);
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    base += k < w ? s_w[k] : 0u;
    all += s_w[k];
  }
  __syncthreads();
  if (total) *total = all;
  return base + inc - v;
}

// the same sum of one uint64 per thread (s_w: NT / 64 uint64 words)
__device__ __forceinline__ uint64_t wave_incl_add64(uint64_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up((unsigned long long)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

template <int NT>
__device__ __forceinline__ uint64_t block_excl_add64(uint64_t v, uint64_t* s_w,
                                                     uint64_t* total = nullptr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t inc = wave_incl_add64(v, lane);
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  uint64_t base = 0, all = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    base += k < w ? s_w[k] : 0ull;
    all += s_w[k];
  }
  __syncthreads();
  if (total) *total = all;
  return base + inc - v;
}

// exclusive running maximum (identity 0) likewise
template <int NT>
__device__ __forceinline__ uint32_t block_excl_max(uint32_t v, uint32_t* s_w,
                                                   uint32_t* total = nullptr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_max(v, lane);
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    base = max(base, k < w ? s_w[k] : 0u);
    all = max(all, s_w[k]);
  }
  __syncthreads();
  if (total) *total = all;
  const uint32_t prev = __shfl_up(inc, 1, 64);
  return max(base, lane ? prev : 0u);
}

// One workgroup of NT threads: exclusive sum of a[0 .. n) in place, in trips
// of NT with a carry; returns the total.  s_w as above.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_add_array(uint32_t* __restrict__ a, int64_t n,
                                                         uint32_t* s_w) {
  uint32_t carry = 0;
  for (int64_t c0 = 0; c0 < n; c0 += NT) {
    const int64_t c = c0 + threadIdx.x;
    const uint32_t v = c < n ? a[c] : 0u;
    uint32_t total = 0;
    const uint32_t ex = block_excl_add<NT>(v, s_w, &total);
    if (c < n) a[c] = carry + ex;
    carry += total;
  }
  return carry;
}

// Orders this wave's LDS writes before its later LDS reads (no workgroup
// barrier: the waves work on disjoint words).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t lanemask_lt(int lane) { return (1ull << lane) - 1ull; }

// lanes of `active` holding the same `bits`-bit value as this lane
__device__ __forceinline__ uint64_t match_peers(uint32_t d, bool active, int bits) {
  uint64_t peers = __ballot(active);
  for (int b = 0; b < bits; ++b) {
    const bool set = (d >> b) & 1u;
    const uint64_t m = __ballot(active && set);
    peers &= set ? m : ~m;
  }
  return peers;
}

}  // namespace s3
