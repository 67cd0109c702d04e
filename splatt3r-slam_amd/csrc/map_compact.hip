// Map compaction (include/s3v.h): merge the Gaussians of each voxel.
//
//   k_mc_keys        voxel key of every live row (dropped rows: all ones),
//                    dropped count, the occupied cell range (k_mc_range)
//   k_mc_pack        keys packed to that range, order kept, dropped rows
//                    behind every group; the index column of the sort
//   sort             stable LSD radix sort of (key, index), up to eight 8-bit
//                    passes: k_mc_hist -> k_mc_row_scan -> k_mc_scatter
//                    (the shared pass of radix_pass.hpp with 64-bit keys); all
//                    eight are launched, those past the packed width return
//   k_mc_heads       group heads in sorted order; the head flag of each input
//                    row; group = -1 of the dropped rows
//   k_mc_scan_*      two scans in the same three launches: the running
//                    maximum of the head positions (every sorted position's
//                    group start) and the exclusive sum of the head flags in
//                    input order (the output row of each group: ordered by
//                    the group's lowest input index)
//   k_mc_reduce      one thread per chunk of <= 64 consecutive members of a
//                    group: a group of one chunk is finished here, the others
//                    leave one partial per chunk
//   k_mc_long        one workgroup per group of more than one chunk
//
// Every sum is double in an order the input alone fixes (s3v.h); there is no
// floating-point atomic (the two counters are integers).
#include <algorithm>
#include "common.hpp"
#include "radix_pass.hpp"
#include "s3v.h"

namespace {

constexpr int kT = 256;               // threads of every kernel but the top scan
constexpr int kPer = 8;               // items per thread of a sort or scan block
constexpr int kSeg = kT * kPer;       // 2048 items per block
constexpr int kBits = 8;
constexpr int kBins = 1 << kBits;     // == kT: one digit per thread
constexpr int kPasses = 8;            // 64 key bits
constexpr int kChunk = 64;            // members one thread sums
constexpr int kTerms = 14;            // 1, d[3], S[6], c[3], o
constexpr int kSums = 2 * kTerms;     // opacity-weighted, then unweighted
constexpr int kTop = 1024;            // threads of the top scan
constexpr int kLongGrid = 2048;       // most workgroups of k_mc_long
constexpr int64_t kMaxRows = (1ll << 31) - kSeg;
constexpr uint64_t kDroppedKey = ~0ull;
constexpr double kBias = 1048576.0;   // 2^20
constexpr double kTopCell = 2097151.0;
// words of the workspace's `meta`
constexpr int kLo = 0, kHi = 3, kNLong = 6, kMeta = 8;

static_assert(kBins == kT, "one digit per thread");

struct In {
  const float* means;
  const float* cov;
  const float* colors;
  const float* opac;
  const int32_t* kf;
};
struct Out {
  float* means;
  float* cov;
  float* colors;
  float* opac;
  int32_t* kf;
};

__device__ __forceinline__ int64_t live_n(const int64_t* n_dev, int64_t n_max) {
  if (!n_dev) return n_max;
  const int64_t n = *n_dev;
  return n < 0 ? 0 : (n < n_max ? n : n_max);
}

__device__ __forceinline__ uint64_t cell(float x, double origin, double voxel) {
  double t = floor(((double)x - origin) / voxel) + kBias;
  t = t < 0.0 ? 0.0 : (t > kTopCell ? kTopCell : t);
  return (uint64_t)t;
}

// One workgroup per kSeg rows: the keys, the dropped count and the block's
// occupied cell range (blk[6 b ..]: lowest x y z, highest x y z), which
// k_mc_range folds into meta: no atomic on the range (one per wave on six
// words took longer than the whole sort).
__global__ void __launch_bounds__(kT)
k_mc_keys(In in, const int64_t* __restrict__ n_dev, int64_t n_max, double ox, double oy,
          double oz, double voxel, uint64_t* __restrict__ keys,
          unsigned long long* __restrict__ dropped, uint32_t* __restrict__ blk) {
  __shared__ uint32_t s_r[kT / 64][6];
  const int64_t n = live_n(n_dev, n_max);
  uint32_t r[6] = {~0u, ~0u, ~0u, 0u, 0u, 0u};
  uint32_t nbad = 0;
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = (int64_t)blockIdx.x * kSeg + j * kT + threadIdx.x;
    if (i >= n) break;
    const float x = in.means[3 * i], y = in.means[3 * i + 1], z = in.means[3 * i + 2];
    bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(in.opac[i]);
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && isfinite(in.cov[6 * i + k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && isfinite(in.colors[3 * i + k]);
    uint64_t key = kDroppedKey;
    if (ok) {
      const uint64_t c[3] = {cell(x, ox, voxel), cell(y, oy, voxel), cell(z, oz, voxel)};
      key = (c[0] << 42) | (c[1] << 21) | c[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        r[k] = min(r[k], (uint32_t)c[k]);
        r[3 + k] = max(r[3 + k], (uint32_t)c[k]);
      }
    } else {
      ++nbad;
    }
    keys[i] = key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = min(r[k], (uint32_t)__shfl_xor(r[k], o, 64));
      r[3 + k] = max(r[3 + k], (uint32_t)__shfl_xor(r[3 + k], o, 64));
    }
    nbad += __shfl_xor(nbad, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (nbad) atomicAdd(dropped, (unsigned long long)nbad);
#pragma unroll
    for (int k = 0; k < 6; ++k) s_r[threadIdx.x >> 6][k] = r[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    uint32_t v = s_r[0][k];
    for (int w = 1; w < kT / 64; ++w) v = k < 3 ? min(v, s_r[w][k]) : max(v, s_r[w][k]);
    blk[(size_t)blockIdx.x * 6 + k] = v;
  }
}

// one workgroup: the blocks' ranges -> meta[kLo ..], meta[kHi ..]
__global__ void __launch_bounds__(kTop)
k_mc_range(const uint32_t* __restrict__ blk, int64_t nblk, uint32_t* __restrict__ meta) {
  __shared__ uint32_t s_r[kTop / 64][6];
  uint32_t r[6] = {~0u, ~0u, ~0u, 0u, 0u, 0u};
  for (int64_t b = threadIdx.x; b < nblk; b += kTop) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = min(r[k], blk[b * 6 + k]);
      r[3 + k] = max(r[3 + k], blk[b * 6 + 3 + k]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = min(r[k], (uint32_t)__shfl_xor(r[k], o, 64));
      r[3 + k] = max(r[3 + k], (uint32_t)__shfl_xor(r[3 + k], o, 64));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_r[threadIdx.x >> 6][k] = r[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    uint32_t v = s_r[0][k];
    for (int w = 1; w < kTop / 64; ++w) v = k < 3 ? min(v, s_r[w][k]) : max(v, s_r[w][k]);
    meta[(k < 3 ? kLo : kHi - 3) + k] = v;
  }
}

// The sort keys are the cells relative to the lowest occupied cell of each
// axis, packed to the bits the occupied range needs (the order of the full
// keys is kept), a dropped row one bit above: a scene a few thousand voxels
// across sorts in four passes instead of eight.
struct Plan {
  uint32_t lo[3];
  int bits[3];    // per axis
  int total;      // + 1 with a dropped row
  int passes;
};

__device__ __forceinline__ Plan plan_of(const uint32_t* __restrict__ meta,
                                        const unsigned long long* __restrict__ dropped) {
  Plan p;
  p.total = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t lo = meta[kLo + k], hi = meta[kHi + k];
    p.lo[k] = lo;
    p.bits[k] = hi > lo ? 32 - __clz((int)(hi - lo)) : 0;
    p.total += p.bits[k];
  }
  if (*dropped) ++p.total;
  p.passes = (p.total + kBits - 1) / kBits;
  return p;
}

__global__ void __launch_bounds__(kT)
k_mc_pack(const int64_t* __restrict__ n_dev, int64_t n_max, const uint32_t* __restrict__ meta,
          const unsigned long long* __restrict__ dropped, uint64_t* __restrict__ keys,
          uint32_t* __restrict__ vals) {
  const int64_t n = live_n(n_dev, n_max);
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const Plan p = plan_of(meta, dropped);
  const uint64_t key = keys[i];
  uint64_t packed;
  if (key == kDroppedKey) {
    packed = 1ull << (p.total - 1);
  } else {
    const uint64_t cx = (key >> 42) - p.lo[0], cy = ((key >> 21) & 0x1FFFFFull) - p.lo[1],
                   cz = (key & 0x1FFFFFull) - p.lo[2];
    packed = (cx << (p.bits[1] + p.bits[2])) | (cy << p.bits[2]) | cz;
  }
  keys[i] = packed;
  vals[i] = (uint32_t)i;
}

// ---------------------------------------------------------------- sort ----
// The bodies of a pass are radix_pass.hpp's with 64-bit keys and a fixed
// 8-bit digit; a pass past the packed width returns at once.
struct Digit {
  int shift;
  static constexpr int bits = kBits, max_bits = kBits;
  __device__ __forceinline__ uint32_t operator()(uint64_t key) const {
    return (uint32_t)(key >> shift) & (uint32_t)(kBins - 1);
  }
};

// digit counts of every kSeg-item block -> hist[digit][block]
__global__ void __launch_bounds__(kT)
k_mc_hist(const int64_t* __restrict__ n_dev, int64_t n_max, const uint64_t* __restrict__ keys,
          int shift, int64_t nseg, uint32_t* __restrict__ hist,
          const uint32_t* __restrict__ meta, const unsigned long long* __restrict__ dropped) {
  if (shift >= plan_of(meta, dropped).passes * kBits) return;
  s3::radix_hist<kT, kPer, uint64_t, uint64_t>(live_n(n_dev, n_max), keys, Digit{shift}, nseg,
                                               hist);
}

// per digit row: exclusive scan over `cols` blocks in place, row total to tot[row]
__global__ void __launch_bounds__(kT)
k_mc_row_scan(uint32_t* __restrict__ hist, int64_t cols, uint32_t* __restrict__ tot, int shift,
              const uint32_t* __restrict__ meta, const unsigned long long* __restrict__ dropped) {
  if (shift >= plan_of(meta, dropped).passes * kBits) return;
  s3::radix_row_scan<kT, 1>(hist, cols, tot);
}

__global__ void __launch_bounds__(kT)
k_mc_scatter(const int64_t* __restrict__ n_dev, int64_t n_max, const uint64_t* __restrict__ kin,
             const uint32_t* __restrict__ vin, uint64_t* __restrict__ kout,
             uint32_t* __restrict__ vout, int shift, int64_t nseg,
             const uint32_t* __restrict__ hist, const uint32_t* __restrict__ tot,
             const uint32_t* __restrict__ meta, const unsigned long long* __restrict__ dropped) {
  if (shift >= plan_of(meta, dropped).passes * kBits) return;
  const int64_t n = live_n(n_dev, n_max);
  if ((int64_t)blockIdx.x * kSeg >= n) return;
  __builtin_assume(vin != nullptr && kout != nullptr);   // the body's two null options are raster's
  s3::radix_scatter<kT, kPer, uint64_t, uint64_t>(n, kin, vin, kout, vout, Digit{shift}, nseg,
                                                  hist, tot);
}

// ------------------------------------------------------ heads and scans ----
// the two buffer pairs of the sort: an odd number of passes ends in the second
struct Sorted {
  const uint64_t* keys[2];
  const uint32_t* vals[2];
};

__global__ void __launch_bounds__(kT)
k_mc_heads(const int64_t* __restrict__ n_dev, int64_t n_max,
           const unsigned long long* __restrict__ dropped, const uint32_t* __restrict__ meta,
           Sorted sorted, uint32_t* __restrict__ hp, uint32_t* __restrict__ isf,
           int64_t* __restrict__ group) {
  const int side = plan_of(meta, dropped).passes & 1;
  const uint64_t* __restrict__ ks = sorted.keys[side];
  const uint32_t* __restrict__ is = sorted.vals[side];
  const int64_t n = live_n(n_dev, n_max);
  const int64_t nk = n - (int64_t)*dropped;
  const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (j >= n) return;
  const bool head = j < nk && (j == 0 || ks[j] != ks[j - 1]);
  const uint32_t i = is[j];
  hp[j] = head ? (uint32_t)j : 0u;
  isf[i] = head ? 1u : 0u;
  if (j >= nk) group[i] = -1;
}

// block b of kSeg items: the maximum of hp and the sum of isf
__global__ void __launch_bounds__(kT)
k_mc_scan_sums(const int64_t* __restrict__ n_dev, int64_t n_max, const uint32_t* __restrict__ hp,
               const uint32_t* __restrict__ isf, int64_t nblk, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_w[kT / 64];
  const int64_t n = live_n(n_dev, n_max);
  const int64_t i0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
  uint32_t mx = 0, sm = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (i0 + q < n) {
      mx = max(mx, hp[i0 + q]);
      sm += isf[i0 + q];
    }
  uint32_t tmx, tsm;
  s3::block_excl_max<kT>(mx, s_w, &tmx);
  s3::block_excl_add<kT>(sm, s_w, &tsm);
  if (threadIdx.x == 0) {
    bsum[blockIdx.x] = tmx;
    bsum[nblk + blockIdx.x] = tsm;
  }
}

// one workgroup: both rows of bsum scanned exclusively in place, *m = total
__global__ void __launch_bounds__(kTop)
k_mc_scan_top(int64_t nblk, uint32_t* __restrict__ bsum, int64_t* __restrict__ m) {
  __shared__ uint32_t s_w[kTop / 64];
  uint32_t cmx = 0, csm = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += kTop) {
    const int64_t b = b0 + threadIdx.x;
    const uint32_t mx = b < nblk ? bsum[b] : 0u;
    const uint32_t sm = b < nblk ? bsum[nblk + b] : 0u;
    uint32_t tmx, tsm;
    const uint32_t emx = s3::block_excl_max<kTop>(mx, s_w, &tmx);
    const uint32_t esm = s3::block_excl_add<kTop>(sm, s_w, &tsm);
    if (b < nblk) {
      bsum[b] = max(cmx, emx);
      bsum[nblk + b] = csm + esm;
    }
    cmx = max(cmx, tmx);
    csm += tsm;
  }
  if (threadIdx.x == 0) *m = (int64_t)csm;
}

// hp -> inclusive running maximum, isf -> exclusive sum, both in place
__global__ void __launch_bounds__(kT)
k_mc_scan_apply(const int64_t* __restrict__ n_dev, int64_t n_max, uint32_t* __restrict__ hp,
                uint32_t* __restrict__ isf, int64_t nblk, const uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_w[kT / 64];
  const int64_t n = live_n(n_dev, n_max);
  const int64_t i0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
  uint32_t a[kPer], f[kPer], mx = 0, sm = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    a[q] = i0 + q < n ? hp[i0 + q] : 0u;
    f[q] = i0 + q < n ? isf[i0 + q] : 0u;
    mx = max(mx, a[q]);
    sm += f[q];
  }
  uint32_t rmx = max(bsum[blockIdx.x], s3::block_excl_max<kT>(mx, s_w));
  uint32_t rsm = bsum[nblk + blockIdx.x] + s3::block_excl_add<kT>(sm, s_w);
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (i0 + q < n) {
      rmx = max(rmx, a[q]);
      hp[i0 + q] = rmx;
      isf[i0 + q] = rsm;
      rsm += f[q];
    }
}

// ----------------------------------------------------------------- sums ----
struct Acc {
  double v[kSums];
};

__device__ __forceinline__ void acc_row(Acc& a, const In& in, int64_t i, const double (&mu0)[3]) {
  double t[kTerms];
  t[0] = 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) t[1 + k] = (double)in.means[3 * i + k] - mu0[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) t[4 + k] = (double)in.cov[6 * i + k];
  t[4] += t[1] * t[1];
  t[5] += t[1] * t[2];
  t[6] += t[1] * t[3];
  t[7] += t[2] * t[2];
  t[8] += t[2] * t[3];
  t[9] += t[3] * t[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[10 + k] = (double)in.colors[3 * i + k];
  const double o = (double)in.opac[i];
  t[13] = o;
#pragma unroll
  for (int k = 0; k < kTerms; ++k) {
    a.v[k] += o * t[k];
    a.v[kTerms + k] += t[k];
  }
}

// the merged Gaussian of a group's sums -> output row `row`
__device__ __forceinline__ void finish(const Acc& a, const double (&mu0)[3], const Out& out,
                                       int64_t row) {
  const double* s = a.v[0] != 0.0 ? a.v : a.v + kTerms;
  const double W = s[0];
  const double d[3] = {s[1] / W, s[2] / W, s[3] / W};
#pragma unroll
  for (int k = 0; k < 3; ++k) out.means[3 * row + k] = (float)(mu0[k] + d[k]);
  out.cov[6 * row + 0] = (float)(s[4] / W - d[0] * d[0]);
  out.cov[6 * row + 1] = (float)(s[5] / W - d[0] * d[1]);
  out.cov[6 * row + 2] = (float)(s[6] / W - d[0] * d[2]);
  out.cov[6 * row + 3] = (float)(s[7] / W - d[1] * d[1]);
  out.cov[6 * row + 4] = (float)(s[8] / W - d[1] * d[2]);
  out.cov[6 * row + 5] = (float)(s[9] / W - d[2] * d[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) out.colors[3 * row + k] = (float)(s[10 + k] / W);
  out.opac[row] = (float)(s[13] / W);
}

// Chunk partials: a full chunk starting at sorted position j covers exactly
// one multiple of kChunk, ceil(j / kChunk), and full chunks are disjoint; a
// short last chunk of a group of several chunks starts >= kChunk + 1 after
// the previous such chunk, so floor(j / kChunk) is unique among those.
__device__ __forceinline__ double* partial_slot(double* part_full, double* part_tail, int64_t j,
                                                int64_t len) {
  return len == kChunk ? part_full + (size_t)((j + kChunk - 1) / kChunk) * kSums
                       : part_tail + (size_t)(j / kChunk) * kSums;
}

__global__ void __launch_bounds__(kT)
k_mc_reduce(In in, Out out, const int64_t* __restrict__ n_dev, int64_t n_max,
            const unsigned long long* __restrict__ dropped, uint32_t* __restrict__ meta,
            Sorted sorted, const uint32_t* __restrict__ hp, const uint32_t* __restrict__ rank,
            int64_t* __restrict__ first, int64_t* __restrict__ group,
            double* __restrict__ part_full, double* __restrict__ part_tail,
            uint2* __restrict__ longs) {
  const uint32_t* __restrict__ is = sorted.vals[plan_of(meta, dropped).passes & 1];
  const int64_t n = live_n(n_dev, n_max);
  const int64_t nk = n - (int64_t)*dropped;
  const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (j >= nk) return;
  const int64_t s = hp[j];
  const int64_t i0 = is[s];          // the group's lowest input index
  const int64_t row = rank[i0];
  group[is[j]] = row;
  const int64_t r = j - s;
  if (r % kChunk) return;
  int64_t len = 1;
  while (len < kChunk && j + len < nk && (int64_t)hp[j + len] == s) ++len;
  const bool ended = j + len >= nk || (int64_t)hp[j + len] != s;
  if (r == 0) {
    first[row] = i0;
    out.kf[row] = in.kf[i0];
    if (len == 1 && ended) {  // a group of one: bit for bit
#pragma unroll
      for (int k = 0; k < 3; ++k) out.means[3 * row + k] = in.means[3 * i0 + k];
#pragma unroll
      for (int k = 0; k < 6; ++k) out.cov[6 * row + k] = in.cov[6 * i0 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) out.colors[3 * row + k] = in.colors[3 * i0 + k];
      out.opac[row] = in.opac[i0];
      return;
    }
  }
  const double mu0[3] = {(double)in.means[3 * i0], (double)in.means[3 * i0 + 1],
                         (double)in.means[3 * i0 + 2]};
  Acc a;
#pragma unroll
  for (int k = 0; k < kSums; ++k) a.v[k] = 0.0;
  for (int64_t t = 0; t < len; ++t) acc_row(a, in, is[j + t], mu0);
  if (r == 0 && ended) {
    finish(a, mu0, out, row);
    return;
  }
  double* p = partial_slot(part_full, part_tail, j, len);
#pragma unroll
  for (int k = 0; k < kSums; ++k) p[k] = a.v[k];
  if (ended) longs[atomicAdd(&meta[kNLong], 1u)] = make_uint2((uint32_t)s, (uint32_t)(j + len));
}

// a group [s, e) of more than one chunk: its chunk partials summed
__global__ void __launch_bounds__(kT)
k_mc_long(In in, Out out, const unsigned long long* __restrict__ dropped,
          const uint32_t* __restrict__ meta, Sorted sorted, const uint32_t* __restrict__ rank,
          double* __restrict__ part_full, double* __restrict__ part_tail,
          const uint2* __restrict__ longs) {
  const uint32_t* __restrict__ is = sorted.vals[plan_of(meta, dropped).passes & 1];
  constexpr int NW = kT / 64;
  __shared__ double s_a[NW][kSums];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t ng = meta[kNLong];
  for (uint32_t g = blockIdx.x; g < ng; g += gridDim.x) {
    const int64_t s = longs[g].x, e = longs[g].y;
    const int64_t nch = (e - s + kChunk - 1) / kChunk;
    Acc a;
#pragma unroll
    for (int k = 0; k < kSums; ++k) a.v[k] = 0.0;
    for (int64_t c = threadIdx.x; c < nch; c += kT) {
      const int64_t j = s + c * kChunk;
      const double* p = partial_slot(part_full, part_tail, j, min<int64_t>(kChunk, e - j));
#pragma unroll
      for (int k = 0; k < kSums; ++k) a.v[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
      double v = a.v[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      a.v[k] = v;
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) s_a[w][k] = a.v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      Acc t;
#pragma unroll
      for (int k = 0; k < kSums; ++k) {
        double v = s_a[0][k];
#pragma unroll
        for (int q = 1; q < NW; ++q) v += s_a[q][k];
        t.v[k] = v;
      }
      const int64_t i0 = is[s];
      const double mu0[3] = {(double)in.means[3 * i0], (double)in.means[3 * i0 + 1],
                             (double)in.means[3 * i0 + 2]};
      finish(t, mu0, out, (int64_t)rank[i0]);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------ workspace ----
struct Carver {
  char* p;
  size_t used = 0;
  explicit Carver(void* base) : p(static_cast<char*>(base)) {}
  template <typename T>
  T* take(size_t count) {
    T* r = p ? reinterpret_cast<T*>(p + used) : nullptr;
    used += (count * sizeof(T) + 255) / 256 * 256;
    return r;
  }
};

struct Work {
  uint64_t* keys[2];
  uint32_t* vals[2];
  uint32_t *hist, *tot, *bsum, *meta, *blk, *hp, *rank;
  double *part_full, *part_tail;
  uint2* longs;
  size_t bytes;
};

Work carve(void* base, int64_t n) {
  Carver c(base);
  Work w;
  const size_t nseg = (size_t)s3::cdiv(n, kSeg);
  const size_t slots = (size_t)(n / kChunk + 2);
  w.keys[0] = c.take<uint64_t>(n);
  w.keys[1] = c.take<uint64_t>(n);
  w.vals[0] = c.take<uint32_t>(n);
  w.vals[1] = c.take<uint32_t>(n);
  w.hist = c.take<uint32_t>((size_t)kBins * nseg);
  w.tot = c.take<uint32_t>(kBins);
  w.bsum = c.take<uint32_t>(2 * nseg);
  w.meta = c.take<uint32_t>(kMeta);
  w.blk = c.take<uint32_t>(6 * nseg);
  w.hp = c.take<uint32_t>(n);
  w.rank = c.take<uint32_t>(n);
  w.part_full = c.take<double>(slots * kSums);
  w.part_tail = c.take<double>(slots * kSums);
  w.longs = c.take<uint2>((size_t)(n / (kChunk + 1) + 2));
  w.bytes = c.used;
  return w;
}

bool is_finite(double v) { return v - v == 0.0; }

}  // namespace

extern "C" size_t s3v_merge_workspace_bytes(int64_t n_max) {
  if (n_max <= 0 || n_max > kMaxRows) return 0;
  return carve(nullptr, n_max).bytes;
}

extern "C" int s3v_merge(const s3v_in* in, const int64_t* n_dev, int64_t n_max,
                         const double* origin, double voxel, const s3v_out* out, int64_t* first,
                         int64_t* group, int64_t* m, int64_t* dropped, void* workspace,
                         size_t workspace_bytes, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n_max >= 0, "s3v_merge: n_max < 0");
  S3_REQUIRE(n_max <= kMaxRows, "s3v_merge: n_max too large");
  S3_REQUIRE(origin && is_finite(origin[0]) && is_finite(origin[1]) && is_finite(origin[2]),
             "s3v_merge: origin must be three finite doubles");
  S3_REQUIRE(voxel > 0.0 && is_finite(voxel), "s3v_merge: voxel must be > 0 and finite");
  S3_REQUIRE(m && dropped, "s3v_merge: null counter");
  hipStream_t st = s3::as_stream(stream);
  S3_HIP(hipMemsetAsync(dropped, 0, sizeof(int64_t), st));
  if (n_max == 0) {
    S3_HIP(hipMemsetAsync(m, 0, sizeof(int64_t), st));
    return S3_OK;
  }
  S3_REQUIRE(in && out && first && group, "s3v_merge: null argument");
  S3_REQUIRE(in->means && in->cov_triu && in->colors && in->opacities && in->kf_id,
             "s3v_merge: null input field");
  S3_REQUIRE(out->means && out->cov_triu && out->colors && out->opacities && out->kf_id,
             "s3v_merge: null output field");
  S3_REQUIRE(out->means != in->means && out->cov_triu != in->cov_triu &&
                 out->colors != in->colors && out->opacities != in->opacities &&
                 out->kf_id != in->kf_id,
             "s3v_merge: the outputs must be distinct from the inputs");
  S3_REQUIRE(workspace && workspace_bytes >= s3v_merge_workspace_bytes(n_max),
             "s3v_merge: workspace too small");
  S3_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 256 == 0,
             "s3v_merge: workspace must be 256-byte aligned");
  const Work w = carve(workspace, n_max);
  const In i{in->means, in->cov_triu, in->colors, in->opacities, in->kf_id};
  const Out o{out->means, out->cov_triu, out->colors, out->opacities, out->kf_id};
  auto* drop = reinterpret_cast<unsigned long long*>(dropped);
  const int64_t nseg = s3::cdiv(n_max, kSeg);
  const unsigned rows = (unsigned)s3::cdiv(n_max, kT);

  S3_HIP(hipMemsetAsync(w.meta, 0, kMeta * sizeof(uint32_t), st));
  k_mc_keys<<<(unsigned)nseg, kT, 0, st>>>(i, n_dev, n_max, origin[0], origin[1], origin[2],
                                           voxel, w.keys[0], drop, w.blk);
  k_mc_range<<<1, kTop, 0, st>>>(w.blk, nseg, w.meta);
  k_mc_pack<<<rows, kT, 0, st>>>(n_dev, n_max, w.meta, drop, w.keys[0], w.vals[0]);
  S3_LAUNCH_CHECK();
  // every pass is launched; those past the packed keys' width return at once
  for (int p = 0; p < kPasses; ++p) {
    const int src = p & 1, shift = p * kBits;
    k_mc_hist<<<(unsigned)nseg, kT, 0, st>>>(n_dev, n_max, w.keys[src], shift, nseg, w.hist,
                                             w.meta, drop);
    k_mc_row_scan<<<kBins, kT, 0, st>>>(w.hist, nseg, w.tot, shift, w.meta, drop);
    k_mc_scatter<<<(unsigned)nseg, kT, 0, st>>>(n_dev, n_max, w.keys[src], w.vals[src],
                                                 w.keys[1 - src], w.vals[1 - src], shift, nseg,
                                                 w.hist, w.tot, w.meta, drop);
    S3_LAUNCH_CHECK();
  }
  const Sorted sorted{{w.keys[0], w.keys[1]}, {w.vals[0], w.vals[1]}};
  uint32_t *hp = w.hp, *rank = w.rank;
  k_mc_heads<<<rows, kT, 0, st>>>(n_dev, n_max, drop, w.meta, sorted, hp, rank, group);
  k_mc_scan_sums<<<(unsigned)nseg, kT, 0, st>>>(n_dev, n_max, hp, rank, nseg, w.bsum);
  k_mc_scan_top<<<1, kTop, 0, st>>>(nseg, w.bsum, m);
  k_mc_scan_apply<<<(unsigned)nseg, kT, 0, st>>>(n_dev, n_max, hp, rank, nseg, w.bsum);
  S3_LAUNCH_CHECK();
  k_mc_reduce<<<rows, kT, 0, st>>>(i, o, n_dev, n_max, drop, w.meta, sorted, hp, rank, first,
                                   group, w.part_full, w.part_tail, w.longs);
  const unsigned lg = (unsigned)std::min<int64_t>(kLongGrid, n_max / (kChunk + 1) + 1);
  k_mc_long<<<lg, kT, 0, st>>>(i, o, drop, w.meta, sorted, rank, w.part_full, w.part_tail,
                               w.longs);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
