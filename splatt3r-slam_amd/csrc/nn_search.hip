// Exact nearest neighbour on a uniform grid, distance statistics and
// area-uniform mesh sampling (include/s3k.h; arithmetic: nn_search_math.hpp).
//
//   build   k_nn_count       cell id of every row, counts per cell (integer
//                            atomics), dropped rows
//           k_nn_scan_*      exclusive sums of the counts -> start (three
//                            launches over segments of 2,048 cells)
//           k_nn_fill        records into their cells (slot = start + an
//                            integer atomic on the cell's cursor)
//   query   k_nn_qkeys       cell id of every query (non-finite rows: one past
//                            the last cell)
//           sort             stable LSD radix sort of (cell id, query index):
//                            the shared pass of radix_pass.hpp with 32-bit
//                            keys, as many 8-bit passes as the cell ids need
//           k_nn_query       one thread per query in cell order:
//                            s3k::search, result written to the query's own row
//           k_nn_query_wave  the same with one wave per query, and k_nn_query
//                            without the sort: s3k_set_query_mode, measured and
//                            not chosen, kept for the benchmark
//   knn     k_nn_qkeys, sort  as the query
//           k_nn_knn<CAP>    one thread per query in cell order: s3k::search_k
//                            with CAP = 4, 8, 16 or 32 register slots (the
//                            smallest that holds k), the k slots and the two
//                            row means written to the query's own row
//   stats   k_nn_stats_part, k_nn_stats_final      fixed-order double sums
//   sample  k_nn_area        face areas, bad faces, A_max (atomicMax on the
//                            bits of a non-negative double: an integer atomic)
//           k_nn_w*          inclusive uint64 sums of the weights
//           k_nn_sample      one thread per sample
//
// There is no floating-point atomic; the order of the records inside a cell
// is the only thing the atomics leave open, and no result depends on it.
#include <algorithm>
#include <atomic>
#include "arg_check.hpp"
#include "common.hpp"
#include "nn_search_math.hpp"
#include "radix_pass.hpp"
#include "s3k.h"

namespace {

constexpr int kT = 256;               // threads of every kernel but the top scans
constexpr int kPer = 8;               // items per thread of a sort or scan block
constexpr int kSeg = kT * kPer;       // 2048 items per block
constexpr int kBits = 8;
constexpr int kBins = 1 << kBits;     // == kT: one digit per thread
constexpr int kTop = 1024;            // threads of the top scans
constexpr int kStats = 5;
constexpr int64_t kMaxRows = (1ll << 31) - kSeg;
constexpr int64_t kMaxStats = ((1ll << 31) - 1) * kSeg;   // the grid of k_nn_stats_part
constexpr uint32_t kNoCell = ~0u;

static_assert(kBins == kT, "one digit per thread");
static_assert(sizeof(s3k::Rec) == 16, "16-byte records");

// ---------------------------------------------------------------- build ----
__global__ void __launch_bounds__(kT)
k_nn_count(const float* __restrict__ ref, int64_t n, s3k::Grid g, uint32_t* __restrict__ cid,
           uint32_t* __restrict__ count, unsigned long long* __restrict__ dropped) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const float x = ref[3 * i], y = ref[3 * i + 1], z = ref[3 * i + 2];
    uint32_t id = kNoCell;
    if (s3k::finite3(x, y, z)) {
      id = (uint32_t)s3k::cell_of(g, x, y, z);
      atomicAdd(&count[id], 1u);
    } else {
      bad = true;
    }
    cid[i] = id;
  }
  const uint64_t b = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(dropped, (unsigned long long)__popcll(b));
}

// block b of kSeg cells: the sum of its counts
__global__ void __launch_bounds__(kT)
k_nn_scan_sums(const uint32_t* __restrict__ count, int64_t cells, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_w[kT / 64];
  const int64_t i0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
  uint32_t sm = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (i0 + q < cells) sm += count[i0 + q];
  uint32_t total;
  s3::block_excl_add<kT>(sm, s_w, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum scanned exclusively in place, *total = the sum
__global__ void __launch_bounds__(kTop)
k_nn_scan_top(uint32_t* __restrict__ bsum, int64_t nblk, uint32_t* __restrict__ total) {
  __shared__ uint32_t s_w[kTop / 64];
  const uint32_t all = s3::block_excl_add_array<kTop>(bsum, nblk, s_w);
  if (threadIdx.x == 0) *total = all;
}

// count -> start (exclusive), count cleared: it is the cursor of k_nn_fill
__global__ void __launch_bounds__(kT)
k_nn_scan_apply(uint32_t* __restrict__ count, int64_t cells, const uint32_t* __restrict__ bsum,
                uint32_t* __restrict__ start) {
  __shared__ uint32_t s_w[kT / 64];
  const int64_t i0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
  uint32_t a[kPer], sm = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    a[q] = i0 + q < cells ? count[i0 + q] : 0u;
    sm += a[q];
  }
  uint32_t run = bsum[blockIdx.x] + s3::block_excl_add<kT>(sm, s_w);
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (i0 + q < cells) {
      start[i0 + q] = run;
      count[i0 + q] = 0u;
      run += a[q];
    }
}

__global__ void __launch_bounds__(kT)
k_nn_fill(const float* __restrict__ ref, int64_t n, const uint32_t* __restrict__ cid,
          const uint32_t* __restrict__ start, uint32_t* __restrict__ cursor,
          s3k::Rec* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = cid[i];
  if (id == kNoCell) return;
  const uint32_t slot = start[id] + atomicAdd(&cursor[id], 1u);
  rec[slot] = s3k::Rec{ref[3 * i], ref[3 * i + 1], ref[3 * i + 2], (int32_t)i};
}

// ---------------------------------------------------------------- query ----
__global__ void __launch_bounds__(kT)
k_nn_qkeys(const float* __restrict__ q, int64_t m, s3k::Grid g, uint32_t* __restrict__ keys,
           uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= m) return;
  const float x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
  keys[i] = s3k::finite3(x, y, z) ? (uint32_t)s3k::cell_of(g, x, y, z) : (uint32_t)s3k::cells_of(g);
  vals[i] = (uint32_t)i;
}

struct Digit {
  int shift;
  static constexpr int bits = kBits, max_bits = kBits;
  __device__ __forceinline__ uint32_t operator()(uint32_t key) const {
    return (key >> shift) & (uint32_t)(kBins - 1);
  }
};

__global__ void __launch_bounds__(kT)
k_nn_hist(int64_t m, const uint32_t* __restrict__ keys, int shift, int64_t nseg,
          uint32_t* __restrict__ hist) {
  s3::radix_hist<kT, kPer, uint32_t, uint32_t>(m, keys, Digit{shift}, nseg, hist);
}

__global__ void __launch_bounds__(kT)
k_nn_row_scan(uint32_t* __restrict__ hist, int64_t cols, uint32_t* __restrict__ tot) {
  s3::radix_row_scan<kT, 1>(hist, cols, tot);
}

__global__ void __launch_bounds__(kT)
k_nn_scatter(int64_t m, const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
             uint32_t* __restrict__ kout, uint32_t* __restrict__ vout, int shift, int64_t nseg,
             const uint32_t* __restrict__ hist, const uint32_t* __restrict__ tot) {
  __builtin_assume(vin != nullptr && kout != nullptr);   // the body's two null options are raster's
  s3::radix_scatter<kT, kPer, uint32_t, uint32_t>(m, kin, vin, kout, vout, Digit{shift}, nseg,
                                                  hist, tot);
}

__global__ void __launch_bounds__(kT)
k_nn_query(s3k::Grid g, const float* __restrict__ q, const uint32_t* __restrict__ order, int64_t m,
           double max_dist, int32_t* __restrict__ idx, float* __restrict__ dist) {
  const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (j >= m) return;
  const int64_t i = order ? order[j] : j;      // null: the queries' own order (A/B)
  const s3k::Hit h = s3k::search(g, q[3 * i], q[3 * i + 1], q[3 * i + 2], max_dist, nullptr);
  idx[i] = h.i;
  dist[i] = (float)sqrt(h.d2);
}

// the 64 lanes of a wave on one query: lane l takes records l, l + 64, .. of a run
struct WaveLanes {
  int lane;
  __device__ __forceinline__ uint32_t first() const { return (uint32_t)lane; }
  __device__ __forceinline__ uint32_t step() const { return 64u; }
  __device__ __forceinline__ void reduce(s3k::Hit& h) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double d2 = __shfl_xor(h.d2, o, 64);
      const int32_t i = __shfl_xor(h.i, o, 64);
      if (d2 < h.d2 || (d2 == h.d2 && i < h.i)) {
        h.d2 = d2;
        h.i = i;
      }
    }
  }
};

// A/B (s3k_set_query_mode 2): one wave per query, in cell order
__global__ void __launch_bounds__(kT)
k_nn_query_wave(s3k::Grid g, const float* __restrict__ q, const uint32_t* __restrict__ order,
                int64_t m, double max_dist, int32_t* __restrict__ idx, float* __restrict__ dist) {
  const int64_t j = ((int64_t)blockIdx.x * kT + threadIdx.x) >> 6;
  if (j >= m) return;
  const int64_t i = order[j];
  const WaveLanes lanes{(int)(threadIdx.x & 63)};
  const s3k::Hit h = s3k::search(g, q[3 * i], q[3 * i + 1], q[3 * i + 2], max_dist, nullptr, lanes);
  if (lanes.lane == 0) {
    idx[i] = h.i;
    dist[i] = (float)sqrt(h.d2);
  }
}

// k nearest rows of each query: any of the four outputs may be null
template <int CAP>
__global__ void __launch_bounds__(kT)
k_nn_knn(s3k::Grid g, const float* __restrict__ q, const uint32_t* __restrict__ order, int64_t m,
         int32_t k, int32_t exclude_self, double max_dist, int32_t* __restrict__ idx,
         float* __restrict__ dist, float* __restrict__ mean_d, float* __restrict__ mean_d2) {
  const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (j >= m) return;
  const int64_t i = order[j];
  s3k::HitK<CAP> h;
  s3k::search_k(g, q[3 * i], q[3 * i + 1], q[3 * i + 2], k, exclude_self ? (int32_t)i : -1,
                max_dist, h, nullptr);
  const s3k::RowStats o = s3k::emit_k(h, k, idx ? idx + i * k : nullptr,
                                      dist ? dist + i * k : nullptr);
  if (mean_d) mean_d[i] = o.mean_d;
  if (mean_d2) mean_d2[i] = o.mean_d2;
}

// ---------------------------------------------------------------- stats ----
// pairwise tree over the workgroup's kT values of each statistic: sums for
// 0..3, the maximum for 4; the result in s[k][0]
__device__ __forceinline__ void stats_tree(double (&s)[kStats][kT], const double (&v)[kStats]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kStats; ++k) s[k][t] = v[k];
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < kStats - 1; ++k) s[k][t] += s[k][t + o];
      s[kStats - 1][t] = fmax(s[kStats - 1][t], s[kStats - 1][t + o]);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kT)
k_nn_stats_part(const float* __restrict__ dist, int64_t m, double threshold,
                double* __restrict__ part) {
  __shared__ double s[kStats][kT];
  const int64_t i0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
  double v[kStats] = {0.0, 0.0, 0.0, 0.0, -(double)INFINITY};
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (i0 + q < m) {
      const float f = dist[i0 + q];
      if (fabsf(f) <= s3k::kFltMax) {
        const double d = (double)f;
        v[0] += 1.0;
        v[1] += d;
        v[2] += d * d;
        v[3] += d <= threshold ? 1.0 : 0.0;
        v[4] = fmax(v[4], d);
      }
    }
  stats_tree(s, v);
  if (threadIdx.x < kStats) part[(size_t)blockIdx.x * kStats + threadIdx.x] = s[threadIdx.x][0];
}

__global__ void __launch_bounds__(kT)
k_nn_stats_final(const double* __restrict__ part, int64_t nblk, double* __restrict__ out) {
  __shared__ double s[kStats][kT];
  double v[kStats] = {0.0, 0.0, 0.0, 0.0, -(double)INFINITY};
  for (int64_t b = threadIdx.x; b < nblk; b += kT) {
#pragma unroll
    for (int k = 0; k < kStats - 1; ++k) v[k] += part[b * kStats + k];
    v[kStats - 1] = fmax(v[kStats - 1], part[b * kStats + kStats - 1]);
  }
  stats_tree(s, v);
  if (threadIdx.x < kStats) out[threadIdx.x] = s[threadIdx.x][0];
}

// --------------------------------------------------------------- sample ----
__global__ void __launch_bounds__(kT)
k_nn_area(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
          double* __restrict__ area, unsigned long long* __restrict__ amax_bits,
          unsigned long long* __restrict__ bad) {
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  bool is_bad = false;
  double a = 0.0;
  if (f < F) {
    a = s3k::checked_area(verts, V, faces, f, &is_bad);
    area[f] = a;
  }
  // areas are >= 0: their bit patterns order like the values
  unsigned long long bits = (unsigned long long)__double_as_longlong(a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits = max(bits, __shfl_xor(bits, o, 64));
  const uint64_t b = __ballot(is_bad);
  if ((threadIdx.x & 63) == 0) {
    if (bits) atomicMax(amax_bits, bits);
    if (b) atomicAdd(bad, (unsigned long long)__popcll(b));
  }
}

__device__ __forceinline__ uint64_t weight_at(const double* __restrict__ area, int64_t f, int64_t F,
                                              double a_max) {
  return f < F ? s3k::face_weight(area[f], a_max) : 0ull;
}

__global__ void __launch_bounds__(kT)
k_nn_wsum(const double* __restrict__ area, int64_t F,
          const unsigned long long* __restrict__ amax_bits, uint64_t* __restrict__ bsum) {
  __shared__ uint64_t s_w[kT / 64];
  const double a_max = __longlong_as_double((long long)*amax_bits);
  const int64_t i0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
  uint64_t sm = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) sm += weight_at(area, i0 + q, F, a_max);
  uint64_t total;
  s3::block_excl_add64<kT>(sm, s_w, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum scanned exclusively in place, *total = Q
__global__ void __launch_bounds__(kTop)
k_nn_wtop(uint64_t* __restrict__ bsum, int64_t nblk, int64_t* __restrict__ total) {
  __shared__ uint64_t s_w[kTop / 64];
  uint64_t carry = 0;
  for (int64_t c0 = 0; c0 < nblk; c0 += kTop) {
    const int64_t c = c0 + threadIdx.x;
    const uint64_t v = c < nblk ? bsum[c] : 0ull;
    uint64_t all = 0;
    const uint64_t ex = s3::block_excl_add64<kTop>(v, s_w, &all);
    if (c < nblk) bsum[c] = carry + ex;
    carry += all;
  }
  if (threadIdx.x == 0) *total = (int64_t)carry;
}

__global__ void __launch_bounds__(kT)
k_nn_wapply(const double* __restrict__ area, int64_t F,
            const unsigned long long* __restrict__ amax_bits, const uint64_t* __restrict__ bsum,
            uint64_t* __restrict__ C) {
  __shared__ uint64_t s_w[kT / 64];
  const double a_max = __longlong_as_double((long long)*amax_bits);
  const int64_t i0 = (int64_t)blockIdx.x * kSeg + (int64_t)threadIdx.x * kPer;
  uint64_t w[kPer], sm = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    w[q] = weight_at(area, i0 + q, F, a_max);
    sm += w[q];
  }
  uint64_t run = bsum[blockIdx.x] + s3::block_excl_add64<kT>(sm, s_w);
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (i0 + q < F) {
      run += w[q];
      C[i0 + q] = run;
    }
}

__global__ void __launch_bounds__(kT)
k_nn_sample(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t F,
            int64_t S, uint64_t seed, const uint64_t* __restrict__ C,
            const int64_t* __restrict__ total, float* __restrict__ points,
            int32_t* __restrict__ face) {
  const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (k >= S) return;
  const uint64_t Q = (uint64_t)*total;
  if (Q == 0) return;
  double u[4];
  s3k::sample_uniforms(k, seed, u);
  const int64_t f = s3k::pick_face(C, F, s3k::sample_target(k, u[0], S, Q));
  // w_f > 0, so f is a face whose three indices were checked
  const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  float p[3];
  s3k::place(verts + 3 * ia, verts + 3 * ib, verts + 3 * ic, u[1], u[2], p);
  points[3 * k] = p[0];
  points[3 * k + 1] = p[1];
  points[3 * k + 2] = p[2];
  face[k] = (int32_t)f;
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

struct GridW {
  uint32_t* start;
  s3k::Rec* rec;
  uint32_t *count, *cid, *bsum;
  size_t bytes;
};

GridW carve_grid(void* base, int64_t n, int64_t cells) {
  Carver c(base);
  GridW w;
  w.start = c.take<uint32_t>((size_t)cells + 1);
  w.rec = c.take<s3k::Rec>((size_t)n);
  w.count = c.take<uint32_t>((size_t)cells);
  w.cid = c.take<uint32_t>((size_t)n);
  w.bsum = c.take<uint32_t>((size_t)s3::cdiv(cells, kSeg));
  w.bytes = c.used;
  return w;
}

struct QueryW {
  uint32_t* keys[2];
  uint32_t* vals[2];
  uint32_t *hist, *tot;
  size_t bytes;
};

QueryW carve_query(void* base, int64_t m) {
  Carver c(base);
  QueryW w;
  const size_t nseg = (size_t)s3::cdiv(m, kSeg);
  for (int k = 0; k < 2; ++k) w.keys[k] = c.take<uint32_t>((size_t)m);
  for (int k = 0; k < 2; ++k) w.vals[k] = c.take<uint32_t>((size_t)m);
  w.hist = c.take<uint32_t>((size_t)kBins * nseg);
  w.tot = c.take<uint32_t>(kBins);
  w.bytes = c.used;
  return w;
}

struct SampleW {
  double* area;
  uint64_t *C, *bsum;
  unsigned long long* amax_bits;
  size_t bytes;
};

SampleW carve_sample(void* base, int64_t F) {
  Carver c(base);
  SampleW w;
  w.area = c.take<double>((size_t)F);
  w.C = c.take<uint64_t>((size_t)F);
  w.bsum = c.take<uint64_t>((size_t)s3::cdiv(F, kSeg));
  w.amax_bits = c.take<unsigned long long>(1);
  w.bytes = c.used;
  return w;
}

// The queries' indices in the order of their cell (non-finite rows last): the
// keys, then a stable LSD radix sort of (cell id, query index) in w.
const uint32_t* sort_by_cell(const s3k::Grid& g, int64_t cells, const float* q, int64_t m,
                             const QueryW& w, hipStream_t st) {
  const int64_t nseg = s3::cdiv(m, kSeg);
  k_nn_qkeys<<<(unsigned)s3::cdiv(m, kT), kT, 0, st>>>(q, m, g, w.keys[0], w.vals[0]);
  // the keys are 0 .. cells: as many 8-bit passes as `cells` has bits
  int bits = 0;
  while ((cells >> bits) != 0) ++bits;
  const int passes = (bits + kBits - 1) / kBits;
  for (int p = 0; p < passes; ++p) {
    const int src = p & 1, shift = p * kBits;
    k_nn_hist<<<(unsigned)nseg, kT, 0, st>>>(m, w.keys[src], shift, nseg, w.hist);
    k_nn_row_scan<<<kBins, kT, 0, st>>>(w.hist, nseg, w.tot);
    k_nn_scatter<<<(unsigned)nseg, kT, 0, st>>>(m, w.keys[src], w.vals[src], w.keys[1 - src],
                                                 w.vals[1 - src], shift, nseg, w.hist, w.tot);
  }
  return w.vals[passes & 1];
}

bool is_finite(double v) { return v - v == 0.0; }

// 0: sorted, one thread per query (the product); 1: unsorted; 2: sorted, one
// wave per query.  Same bits; kept for tools/bench_nn_search.py.
std::atomic<int> g_query_mode{0};

// 0 unless the dims are those of a grid
int64_t cells_of_dims(int32_t nx, int32_t ny, int32_t nz) {
  if (nx < 1 || ny < 1 || nz < 1) return 0;
  const int64_t xy = (int64_t)nx * ny;
  if (xy > S3K_MAX_CELLS) return 0;
  const int64_t cells = xy * nz;
  return cells > S3K_MAX_CELLS ? 0 : cells;
}

int check_grid_args(const char* fn, int64_t n, const double* origin, double cell, int32_t nx,
                    int32_t ny, int32_t nz) {
  S3_REQUIRE(n >= 0, "%s: n < 0", fn);
  S3_REQUIRE(n <= kMaxRows, "%s: n too large", fn);
  S3_REQUIRE(origin && is_finite(origin[0]) && is_finite(origin[1]) && is_finite(origin[2]),
             "%s: origin must be three finite doubles", fn);
  S3_REQUIRE(cell > 0.0 && is_finite(cell), "%s: cell must be > 0 and finite", fn);
  S3_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: every dimension must be >= 1", fn);
  S3_REQUIRE(cells_of_dims(nx, ny, nz) > 0, "%s: more than 2^27 cells", fn);
  return S3_OK;
}

}  // namespace

extern "C" size_t s3k_grid_workspace_bytes(int64_t n, int32_t nx, int32_t ny, int32_t nz) {
  const int64_t cells = cells_of_dims(nx, ny, nz);
  if (n < 0 || n > kMaxRows || cells == 0) return 0;
  return carve_grid(nullptr, n, cells).bytes;
}

extern "C" int s3k_grid_build(const float* ref, int64_t n, const double* origin, double cell,
                              int32_t nx, int32_t ny, int32_t nz, void* grid, size_t grid_bytes,
                              int64_t* dropped, void* stream) {
  s3::clear_error();
  if (int e = check_grid_args("s3k_grid_build", n, origin, cell, nx, ny, nz)) return e;
  S3_REQUIRE(dropped, "s3k_grid_build: null counter");
  S3_REQUIRE(n == 0 || ref, "s3k_grid_build: null ref");
  S3_REQUIRE(grid && grid_bytes >= s3k_grid_workspace_bytes(n, nx, ny, nz),
             "s3k_grid_build: grid workspace too small");
  S3_REQUIRE(s3::aligned(grid, 256), "s3k_grid_build: grid must be 256-byte aligned");
  S3_REQUIRE(n == 0 || !s3::overlap(ref, (size_t)n * 12, grid, grid_bytes),
             "s3k_grid_build: grid overlaps ref");
  const int64_t cells = cells_of_dims(nx, ny, nz);
  const GridW w = carve_grid(grid, n, cells);
  hipStream_t st = s3::as_stream(stream);
  S3_HIP(hipMemsetAsync(dropped, 0, sizeof(int64_t), st));
  if (n == 0) {
    S3_HIP(hipMemsetAsync(w.start, 0, ((size_t)cells + 1) * sizeof(uint32_t), st));
    return S3_OK;
  }
  S3_HIP(hipMemsetAsync(w.count, 0, (size_t)cells * sizeof(uint32_t), st));
  const s3k::Grid g{nullptr, nullptr, origin[0], origin[1], origin[2], cell, nx, ny, nz};
  const unsigned rows = (unsigned)s3::cdiv(n, kT), nblk = (unsigned)s3::cdiv(cells, kSeg);
  k_nn_count<<<rows, kT, 0, st>>>(ref, n, g, w.cid, w.count,
                                  reinterpret_cast<unsigned long long*>(dropped));
  k_nn_scan_sums<<<nblk, kT, 0, st>>>(w.count, cells, w.bsum);
  k_nn_scan_top<<<1, kTop, 0, st>>>(w.bsum, nblk, w.start + cells);
  k_nn_scan_apply<<<nblk, kT, 0, st>>>(w.count, cells, w.bsum, w.start);
  k_nn_fill<<<rows, kT, 0, st>>>(ref, n, w.cid, w.start, w.count, w.rec);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" size_t s3k_query_workspace_bytes(int64_t m) {
  if (m <= 0 || m > kMaxRows) return 0;
  return carve_query(nullptr, m).bytes;
}

extern "C" int s3k_query(const void* grid, size_t grid_bytes, int64_t n, const double* origin,
                         double cell, int32_t nx, int32_t ny, int32_t nz, const float* q, int64_t m,
                         double max_dist, int32_t* idx, float* dist, void* workspace,
                         size_t workspace_bytes, void* stream) {
  s3::clear_error();
  if (int e = check_grid_args("s3k_query", n, origin, cell, nx, ny, nz)) return e;
  S3_REQUIRE(m >= 0, "s3k_query: m < 0");
  S3_REQUIRE(m <= kMaxRows, "s3k_query: m too large");
  S3_REQUIRE(max_dist >= 0.0, "s3k_query: max_dist must be >= 0 or +inf");
  S3_REQUIRE(grid && grid_bytes >= s3k_grid_workspace_bytes(n, nx, ny, nz),
             "s3k_query: grid workspace too small");
  S3_REQUIRE(s3::aligned(grid, 256), "s3k_query: grid must be 256-byte aligned");
  if (m == 0) return S3_OK;
  S3_REQUIRE(q && idx && dist, "s3k_query: null argument");
  S3_REQUIRE(workspace && workspace_bytes >= s3k_query_workspace_bytes(m),
             "s3k_query: workspace too small");
  S3_REQUIRE(s3::aligned(workspace, 256), "s3k_query: workspace must be 256-byte aligned");
  S3_REQUIRE(!s3::overlap(workspace, workspace_bytes, grid, grid_bytes),
             "s3k_query: workspace overlaps the grid");
  {
    const void* arr[3] = {q, idx, dist};
    const size_t len[3] = {(size_t)m * 12, (size_t)m * 4, (size_t)m * 4};
    for (int k = 0; k < 3; ++k) {
      S3_REQUIRE(!s3::overlap(arr[k], len[k], grid, grid_bytes) &&
                     !s3::overlap(arr[k], len[k], workspace, workspace_bytes),
                 "s3k_query: q, idx or dist overlaps the grid or the workspace");
      for (int j = k + 1; j < 3; ++j)
        S3_REQUIRE(!s3::overlap(arr[k], len[k], arr[j], len[j]),
                   "s3k_query: q, idx and dist overlap each other");
    }
  }
  const int64_t cells = cells_of_dims(nx, ny, nz);
  const GridW gw = carve_grid(const_cast<void*>(grid), n, cells);
  const QueryW w = carve_query(workspace, m);
  const s3k::Grid g{gw.start, gw.rec, origin[0], origin[1], origin[2], cell, nx, ny, nz};
  hipStream_t st = s3::as_stream(stream);
  const unsigned rows = (unsigned)s3::cdiv(m, kT);
  const int mode = g_query_mode.load();
  if (mode == 1) {
    k_nn_query<<<rows, kT, 0, st>>>(g, q, nullptr, m, max_dist, idx, dist);
    S3_LAUNCH_CHECK();
    return S3_OK;
  }
  const uint32_t* order = sort_by_cell(g, cells, q, m, w, st);
  if (mode == 2)
    k_nn_query_wave<<<(unsigned)s3::cdiv(m, kT / 64), kT, 0, st>>>(g, q, order, m, max_dist, idx,
                                                                  dist);
  else
    k_nn_query<<<rows, kT, 0, st>>>(g, q, order, m, max_dist, idx, dist);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" size_t s3k_knn_workspace_bytes(int64_t m) { return s3k_query_workspace_bytes(m); }

extern "C" int s3k_knn(const void* grid, size_t grid_bytes, int64_t n, const double* origin,
                       double cell, int32_t nx, int32_t ny, int32_t nz, const float* q, int64_t m,
                       int32_t k, int32_t exclude_self, double max_dist, int32_t* idx, float* dist,
                       float* mean_d, float* mean_d2, void* workspace, size_t workspace_bytes,
                       void* stream) {
  s3::clear_error();
  if (int e = check_grid_args("s3k_knn", n, origin, cell, nx, ny, nz)) return e;
  S3_REQUIRE(m >= 0, "s3k_knn: m < 0");
  S3_REQUIRE(m <= kMaxRows, "s3k_knn: m too large");
  S3_REQUIRE(k >= 1 && k <= S3K_MAX_K, "s3k_knn: k must be in 1 .. 32, got %d", (int)k);
  S3_REQUIRE(idx || dist || mean_d || mean_d2, "s3k_knn: every output is null");
  S3_REQUIRE(!exclude_self || m <= n, "s3k_knn: exclude_self with more queries than rows");
  S3_REQUIRE(max_dist >= 0.0, "s3k_knn: max_dist must be >= 0 or +inf");
  S3_REQUIRE(grid && grid_bytes >= s3k_grid_workspace_bytes(n, nx, ny, nz),
             "s3k_knn: grid workspace too small");
  S3_REQUIRE(s3::aligned(grid, 256), "s3k_knn: grid must be 256-byte aligned");
  if (m == 0) return S3_OK;
  S3_REQUIRE(q, "s3k_knn: null q");
  S3_REQUIRE(workspace && workspace_bytes >= s3k_knn_workspace_bytes(m),
             "s3k_knn: workspace too small");
  S3_REQUIRE(s3::aligned(workspace, 256), "s3k_knn: workspace must be 256-byte aligned");
  S3_REQUIRE(!s3::overlap(workspace, workspace_bytes, grid, grid_bytes),
             "s3k_knn: workspace overlaps the grid");
  {
    const void* arr[5] = {q, idx, dist, mean_d, mean_d2};
    const size_t len[5] = {(size_t)m * 12, (size_t)m * k * 4, (size_t)m * k * 4, (size_t)m * 4,
                           (size_t)m * 4};
    for (int a = 0; a < 5; ++a) {
      if (!arr[a]) continue;
      S3_REQUIRE(!s3::overlap(arr[a], len[a], grid, grid_bytes) &&
                     !s3::overlap(arr[a], len[a], workspace, workspace_bytes),
                 "s3k_knn: q or an output overlaps the grid or the workspace");
      for (int b = a + 1; b < 5; ++b)
        S3_REQUIRE(!arr[b] || !s3::overlap(arr[a], len[a], arr[b], len[b]),
                   "s3k_knn: q and the outputs overlap each other");
    }
  }
  const int64_t cells = cells_of_dims(nx, ny, nz);
  const GridW gw = carve_grid(const_cast<void*>(grid), n, cells);
  const QueryW w = carve_query(workspace, m);
  const s3k::Grid g{gw.start, gw.rec, origin[0], origin[1], origin[2], cell, nx, ny, nz};
  hipStream_t st = s3::as_stream(stream);
  const unsigned rows = (unsigned)s3::cdiv(m, kT);
  const uint32_t* order = sort_by_cell(g, cells, q, m, w, st);
#define S3K_KNN(CAP)                                                                          \
  k_nn_knn<CAP><<<rows, kT, 0, st>>>(g, q, order, m, k, exclude_self, max_dist, idx, dist, \
                                     mean_d, mean_d2)
  // the fewest register slots that hold k
  if (k <= 4) S3K_KNN(4);
  else if (k <= 8) S3K_KNN(8);
  else if (k <= 16) S3K_KNN(16);
  else S3K_KNN(32);
#undef S3K_KNN
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" void s3k_set_query_mode(int32_t mode) {
  g_query_mode.store(mode == 1 || mode == 2 ? mode : 0);
}

extern "C" size_t s3k_dist_stats_workspace_bytes(int64_t m) {
  if (m <= 0 || m > kMaxStats) return 0;
  return (size_t)s3::cdiv(m, kSeg) * kStats * sizeof(double);
}

extern "C" int s3k_dist_stats(const float* dist, int64_t m, double threshold, double* out,
                              void* workspace, size_t workspace_bytes, void* stream) {
  s3::clear_error();
  S3_REQUIRE(m >= 0, "s3k_dist_stats: m < 0");
  S3_REQUIRE(m <= kMaxStats, "s3k_dist_stats: m too large");
  S3_REQUIRE(threshold == threshold, "s3k_dist_stats: threshold is NaN");
  S3_REQUIRE(out, "s3k_dist_stats: null output");
  S3_REQUIRE(s3::aligned(out, 8), "s3k_dist_stats: out must be 8-byte aligned");
  hipStream_t st = s3::as_stream(stream);
  const int64_t nblk = s3::cdiv(m, kSeg);
  if (m > 0) {
    S3_REQUIRE(dist, "s3k_dist_stats: null dist");
    S3_REQUIRE(workspace && workspace_bytes >= s3k_dist_stats_workspace_bytes(m),
               "s3k_dist_stats: workspace too small");
    S3_REQUIRE(s3::aligned(workspace, 8), "s3k_dist_stats: workspace must be 8-byte aligned");
    k_nn_stats_part<<<(unsigned)nblk, kT, 0, st>>>(dist, m, threshold,
                                                    static_cast<double*>(workspace));
  }
  k_nn_stats_final<<<1, kT, 0, st>>>(static_cast<const double*>(workspace), nblk, out);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" size_t s3k_sample_workspace_bytes(int64_t n_faces) {
  if (n_faces <= 0 || n_faces > kMaxRows) return 0;
  return carve_sample(nullptr, n_faces).bytes;
}

extern "C" int s3k_sample_mesh(const float* verts, int64_t n_verts, const int32_t* faces,
                               int64_t n_faces, int64_t n_samples, uint64_t seed, float* points,
                               int32_t* face, int64_t* bad, int64_t* total, void* workspace,
                               size_t workspace_bytes, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_samples >= 0, "s3k_sample_mesh: negative count");
  S3_REQUIRE(n_faces <= kMaxRows, "s3k_sample_mesh: too many faces");
  S3_REQUIRE(n_samples <= kMaxRows, "s3k_sample_mesh: too many samples");
  S3_REQUIRE(bad && total, "s3k_sample_mesh: null counter");
  hipStream_t st = s3::as_stream(stream);
  if (n_faces > 0) {
    S3_REQUIRE(faces && (n_verts == 0 || verts), "s3k_sample_mesh: null mesh");
    S3_REQUIRE(n_samples == 0 || (points && face), "s3k_sample_mesh: null output");
    S3_REQUIRE(workspace && workspace_bytes >= s3k_sample_workspace_bytes(n_faces),
               "s3k_sample_mesh: workspace too small");
    S3_REQUIRE(s3::aligned(workspace, 256), "s3k_sample_mesh: workspace must be 256-byte aligned");
  }
  S3_HIP(hipMemsetAsync(bad, 0, sizeof(int64_t), st));
  S3_HIP(hipMemsetAsync(total, 0, sizeof(int64_t), st));
  if (n_faces == 0) return S3_OK;
  const SampleW w = carve_sample(workspace, n_faces);
  S3_HIP(hipMemsetAsync(w.amax_bits, 0, sizeof(unsigned long long), st));
  const unsigned rows = (unsigned)s3::cdiv(n_faces, kT), nblk = (unsigned)s3::cdiv(n_faces, kSeg);
  k_nn_area<<<rows, kT, 0, st>>>(verts, n_verts, faces, n_faces, w.area, w.amax_bits,
                                 reinterpret_cast<unsigned long long*>(bad));
  k_nn_wsum<<<nblk, kT, 0, st>>>(w.area, n_faces, w.amax_bits, w.bsum);
  k_nn_wtop<<<1, kTop, 0, st>>>(w.bsum, nblk, total);
  k_nn_wapply<<<nblk, kT, 0, st>>>(w.area, n_faces, w.amax_bits, w.bsum, w.C);
  if (n_samples > 0)
    k_nn_sample<<<(unsigned)s3::cdiv(n_samples, kT), kT, 0, st>>>(verts, faces, n_faces, n_samples,
                                                                  seed, w.C, total, points, face);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
