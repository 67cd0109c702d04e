// The three kernel bodies of one pass of a segmented stable LSD radix sort.
//
//   radix_hist      digit counts of every segment of NT x PER items ->
//                   hist[digit][segment]
//   radix_row_scan  one workgroup per digit row: exclusive offsets in place,
//                   row total
//   radix_scatter   per-wave digit counts in LDS, the segment's items ranked
//                   within each 64-item window by a ballot match on the digit
//                   (stable by construction), staged in LDS in digit order and
//                   written out as runs of consecutive addresses (a random
//                   scatter of single words would cost one partial-line
//                   write-back per item)
//
// NT threads, PER items per lane, digits of at most log2(NT) bits (thread d
// owns digit d: the per-wave counts of a segment are NT / 64 rows of NT
// words); keys are stored as KS and held in registers as KR; DG is the digit
// functor: dg(KR) -> digit, dg.bits its live width, DG::max_bits the most
// that can be (checked against NT here).  The __global__ kernels
// (names, launch bounds, grids, item counts, early returns) stay with their
// users: raster.hip, map_compact.hip.
#pragma once
#include "wave_scan.hpp"

namespace s3 {

template <int NT, int PER, typename KS, typename KR, typename DG>
__device__ __forceinline__ void radix_hist(int64_t n, const KS* __restrict__ keys, const DG& dg,
                                           int64_t nseg, uint32_t* __restrict__ hist) {
  static_assert((1 << DG::max_bits) <= NT, "one digit per thread");
  __shared__ uint32_t cnt[NT];
  const int d = threadIdx.x, bins = 1 << dg.bits;
  cnt[d] = 0u;
  __syncthreads();
  const int64_t s = blockIdx.x;
  const int64_t i0 = s * (NT * PER);
  KR key[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int64_t i = i0 + j * NT + threadIdx.x;
    key[j] = i < n ? (KR)keys[i] : KR(0);
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    // counts do not depend on the order: one LDS atomic per item (a ballot
    // match per window costs a VALU op per digit bit)
    if (i0 + j * NT + threadIdx.x < n) atomicAdd(&cnt[dg(key[j])], 1u);
  }
  __syncthreads();
  if (d < bins) hist[(size_t)d * nseg + s] = cnt[d];
}

// Per row: exclusive scan over `cols` columns in place, row total to
// tot[row].  Wave w owns a contiguous 1 / NW of the columns: the waves'
// totals first, then the scan with the wave's carry-in, kCh loads in flight
// (a wave scans kCh chunks of 64 columns a trip whether the row has them or
// not: 8 for rows of thousands of segments, 1 for rows of a few hundred).
template <int NT, int kCh>
__device__ __forceinline__ void radix_row_scan(uint32_t* __restrict__ hist, int64_t cols,
                                               uint32_t* __restrict__ tot) {
  constexpr int NW = NT / 64;
  __shared__ uint32_t s_q[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t* h = hist + (size_t)blockIdx.x * cols;
  const int64_t per = (cols + NW - 1) / NW;
  const int64_t q0 = min(cols, (int64_t)w * per), q1 = min(cols, q0 + per);
  uint32_t sum = 0;
  for (int64_t c0 = q0; c0 < q1; c0 += kCh * 64) {
    uint32_t v[kCh];
#pragma unroll
    for (int j = 0; j < kCh; ++j) {
      const int64_t c = c0 + j * 64 + lane;
      v[j] = c < q1 ? h[c] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kCh; ++j) sum += v[j];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) s_q[w] = sum;
  __syncthreads();
  uint32_t carry = 0, all = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    carry += k < w ? s_q[k] : 0u;
    all += s_q[k];
  }
  for (int64_t c0 = q0; c0 < q1; c0 += kCh * 64) {
    uint32_t v[kCh];
#pragma unroll
    for (int j = 0; j < kCh; ++j) {
      const int64_t c = c0 + j * 64 + lane;
      v[j] = c < q1 ? h[c] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kCh; ++j) {
      const int64_t c = c0 + j * 64 + lane;
      const uint32_t inc = wave_incl_add(v[j], lane);
      if (c < q1) h[c] = carry + inc - v[j];
      carry += __shfl(inc, 63, 64);
    }
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = all;
}

// One segment of NT x PER items: wave w owns items [w, w + 1) * 64 * PER of
// it, in PER windows of 64.  vin == nullptr: the value is the item's own
// index; kout == nullptr: the keys are not kept.
template <int NT, int PER, typename KS, typename KR, typename V, typename DG>
__device__ __forceinline__ void radix_scatter(int64_t n, const KS* __restrict__ kin,
                                              const V* __restrict__ vin, KS* __restrict__ kout,
                                              V* __restrict__ vout, const DG& dg, int64_t nseg,
                                              const uint32_t* __restrict__ hist,
                                              const uint32_t* __restrict__ tot) {
  static_assert((1 << DG::max_bits) <= NT, "one digit per thread");
  constexpr int NW = NT / 64, kSeg = NT * PER;
  __shared__ uint32_t cnt[NW][NT];  // per-wave counts -> local slots
  __shared__ uint32_t gdelta[NT];   // global slot - local slot, per digit
  __shared__ uint32_t s_w[NW];
  __shared__ KS sk[kSeg];
  __shared__ V sv[kSeg];
  const int bins = 1 << dg.bits;
#pragma unroll
  for (int k = 0; k < NW; ++k) cnt[k][threadIdx.x] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t s = blockIdx.x;
  const int64_t seg0 = s * kSeg;
  const int64_t base_w = seg0 + (int64_t)w * 64 * PER;
  KR key[PER];
  V val[PER];
  // phase A: every load issued first, then digits and per-wave counts
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int64_t i = base_w + j * 64 + lane;
    key[j] = i < n ? (KR)kin[i] : KR(0);
    val[j] = i < n ? (vin ? vin[i] : (V)i) : V(0);
  }
#pragma unroll
  for (int j = 0; j < PER; ++j)   // counts: order-free, one LDS atomic per item
    if (base_w + j * 64 + lane < n) atomicAdd(&cnt[w][dg(key[j])], 1u);
  __syncthreads();
  // phase B: local slots (digit-major within the segment) and the global
  // offset of each digit's run; thread d owns digit d
  {
    const int d = threadIdx.x;
    uint32_t tb = 0, gt = 0;
    if (d < bins) {
#pragma unroll
      for (int k = 0; k < NW; ++k) tb += cnt[k][d];
      gt = tot[d];
    }
    const uint32_t lbase = block_excl_add<NT>(tb, s_w);
    const uint32_t gbase = block_excl_add<NT>(gt, s_w);
    if (d < bins) {
      gdelta[d] = gbase + hist[(size_t)d * nseg + s] - lbase;
      uint32_t b = lbase;
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        const uint32_t c = cnt[k][d];
        cnt[k][d] = b;
        b += c;
      }
    }
  }
  __syncthreads();
  // phase C: local slot = wave's running slot + rank among equal digits in
  // the window (the last lane of a match group advances the slot); stage key
  // and value there
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const bool ok = base_w + j * 64 + lane < n;
    const uint32_t d = dg(key[j]);
    const uint64_t peers = match_peers(d, ok, dg.bits);
    if (ok) {
      const uint32_t b = cnt[w][d];
      const uint32_t lp = b + (uint32_t)__popcll(peers & lanemask_lt(lane));
      if ((peers >> lane) == 1ull) cnt[w][d] = b + (uint32_t)__popcll(peers);
      sk[lp] = (KS)key[j];
      sv[lp] = val[j];
    }
    wave_lds_sync();
  }
  __syncthreads();
  // phase D: runs of equal digits go to consecutive global slots
  const int m = (int)min<int64_t>(kSeg, n - seg0);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int lp = j * NT + threadIdx.x;
    if (lp < m) {
      const KS k = sk[lp];
      const uint32_t gp = (uint32_t)lp + gdelta[dg((KR)k)];
      if (kout) kout[gp] = k;
      vout[gp] = sv[lp];
    }
  }
}

}  // namespace s3
