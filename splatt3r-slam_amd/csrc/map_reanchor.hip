// Map re-anchor (include/s3a.h): move every Gaussian with its keyframe when
// the keyframe poses change; the arithmetic is map_reanchor_math.hpp.
//
//   k_reanchor_delta  one thread per keyframe: anchor and pose rows in, the
//                     classification and {flag, M[9], t_o[3], t_n[3]} as 16
//                     doubles out, then the new anchor row; the held count,
//                     one integer atomic per wave.
//   k_reanchor_rows   one Gaussian per thread: kf_id[i] and its keyframe's
//                     flag first; a row that does not move ends there with
//                     nothing else loaded or stored (labels come in long runs,
//                     so whole waves and workgroups drop out).  A moved row
//                     reads its 12-byte mean and 24-byte covariance directly
//                     (a wave's lanes cover its rows' bytes exactly once) and
//                     writes them back.  A wave whose moved rows share one
//                     keyframe loads the delta once and broadcasts it.
//   k_reanchor_rows_lds  the same rows, but a workgroup with something to
//                     move stages its 256 rows through LDS as float4 runs
//                     (s3a_set_path(1); kept for the comparison).
//
// No floating-point atomic; the two counters are integers.
#include <atomic>

#include "common.hpp"
#include "map_reanchor_math.hpp"
#include "s3a.h"

namespace {

constexpr int kT = 256;
constexpr int kDelta = s3a::kDelta;
using ull = unsigned long long;

std::atomic<int> g_path{0};

// Add this wave's count of lanes with `hit` to *counter (one atomic per wave
// that has any) and return the wave's ballot.  Every lane of the wave must
// call it.
__device__ __forceinline__ ull wave_count(bool hit, ull* counter) {
  const ull mask = __ballot(hit);
  if (counter && mask && (threadIdx.x & 63) == 0) atomicAdd(counter, (ull)__popcll(mask));
  return mask;
}

__global__ void __launch_bounds__(kT)
k_reanchor_delta(float* __restrict__ anchor, const float* __restrict__ poses, int32_t n_kf,
                 double* __restrict__ delta, ull* __restrict__ held) {
  const int k = blockIdx.x * kT + threadIdx.x;
  bool is_held = false;
  if (k < n_kf) {
    float a[s3a::kPose], p[s3a::kPose];
#pragma unroll
    for (int j = 0; j < s3a::kPose; ++j) {
      a[j] = anchor[k * s3a::kPose + j];
      p[j] = poses[k * s3a::kPose + j];
    }
    double d[kDelta];
    bool adopt;
    is_held = s3a::classify(a, p, d, adopt);
#pragma unroll
    for (int j = 0; j < kDelta; ++j) delta[(int64_t)k * kDelta + j] = d[j];
    if (adopt) {
#pragma unroll
      for (int j = 0; j < s3a::kPose; ++j) anchor[k * s3a::kPose + j] = p[j];
    }
  }
  wave_count(is_held, held);
}

// Does row i move, and under which keyframe?  kf_id and the flag only.
__device__ __forceinline__ bool row_moves(const int32_t* __restrict__ kf_id, int64_t i, int64_t n,
                                          int32_t n_kf, const double* __restrict__ delta,
                                          int32_t& k) {
  k = -1;
  if (i >= n) return false;
  k = kf_id[i];
  if ((uint32_t)k >= (uint32_t)n_kf) return false;
  return delta[(int64_t)k * kDelta] != 0.0;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The delta of every moving lane's keyframe.  Every lane of the wave must
// call it, and at least one must move.  When the moving lanes share one
// keyframe (the common case: labels come in runs) the 16 doubles are loaded
// once, by the wave's first 16 lanes whether their rows move or not, and
// broadcast; otherwise each moving lane loads its own.  The values, and so
// the results, are the same either way.
__device__ __forceinline__ void wave_delta(const double* __restrict__ delta, bool mv, int32_t k,
                                           unsigned long long mask, double (&d)[kDelta]) {
  const int first = __ffsll((long long)mask) - 1;
  const int32_t k0 = __builtin_amdgcn_readlane(k, first);
  if (__all(!mv || k == k0)) {
    const int lane = threadIdx.x & 63;
    double mine = 0.0;
    if (lane < kDelta) mine = delta[(int64_t)k0 * kDelta + lane];
#pragma unroll
    for (int j = 1; j < kDelta; ++j) d[j] = readlane_f64(mine, j);
  } else if (mv) {
    const double* p = delta + (int64_t)k * kDelta;
#pragma unroll
    for (int j = 1; j < kDelta; ++j) d[j] = p[j];
  }
  d[0] = 1.0;
}

__global__ void __launch_bounds__(kT)
k_reanchor_rows(s3w_map m, int32_t n_kf, const double* __restrict__ delta,
                ull* __restrict__ moved) {
  const int64_t n = min(max(*m.n, (int64_t)0), m.cap);
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  int32_t k;
  const bool mv = row_moves(m.kf_id, i, n, n_kf, delta, k);
  const ull mask = wave_count(mv, moved);
  if (!mask) return;   // wave-uniform
  double d[kDelta];
  wave_delta(delta, mv, k, mask, d);
  if (!mv) return;
  float2* __restrict__ cp = reinterpret_cast<float2*>(m.cov_triu) + i * 3;
  float* __restrict__ mp = m.means + i * 3;
  float mu[3] = {mp[0], mp[1], mp[2]};
  const float2 c0 = cp[0], c1 = cp[1], c2 = cp[2];
  float c6[6] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y};
  s3a::move_row(d, mu, c6);
  mp[0] = mu[0];
  mp[1] = mu[1];
  mp[2] = mu[2];
  cp[0] = make_float2(c6[0], c6[1]);
  cp[1] = make_float2(c6[2], c6[3]);
  cp[2] = make_float2(c6[4], c6[5]);
}

// The staged variant: the workgroup's rows are floats [base * 3, base * 3 +
// rows * 3) of means and [base * 6, ...) of cov_triu, both runs starting at a
// multiple of 16 bytes; whole float4s, then at most 3 single floats.  `rows`
// is bounded by the capacity, not the count: rows at or past the count ride
// along and are written back with the bits they had.
__device__ __forceinline__ void run_copy(float* __restrict__ dst, const float* __restrict__ src,
                                         int nfloat, int t) {
  const int nvec = nfloat >> 2;
  float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
  const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
  for (int j = t; j < nvec; j += kT) d4[j] = s4[j];
  const int tail = (nvec << 2) + t;
  if (tail < nfloat) dst[tail] = src[tail];
}

__global__ void __launch_bounds__(kT)
k_reanchor_rows_lds(s3w_map m, int32_t n_kf, const double* __restrict__ delta,
                    ull* __restrict__ moved) {
  __shared__ __attribute__((aligned(16))) float tm[kT * 3];
  __shared__ __attribute__((aligned(16))) float tc[kT * 6];
  const int64_t n = min(max(*m.n, (int64_t)0), m.cap);
  const int64_t base = (int64_t)blockIdx.x * kT;
  const int t = threadIdx.x;
  int32_t k;
  const bool mv = row_moves(m.kf_id, base + t, n, n_kf, delta, k);
  const ull mask = wave_count(mv, moved);
  if (!__syncthreads_or(mv)) return;   // nothing to move: nothing staged
  const int rows = (int)min((int64_t)kT, m.cap - base);
  run_copy(tm, m.means + base * 3, rows * 3, t);
  run_copy(tc, m.cov_triu + base * 6, rows * 6, t);
  __syncthreads();
  double d[kDelta];
  if (mask) wave_delta(delta, mv, k, mask, d);   // wave-uniform
  if (mv) {
    float mu[3] = {tm[t * 3 + 0], tm[t * 3 + 1], tm[t * 3 + 2]};
    float c6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) c6[j] = tc[t * 6 + j];
    s3a::move_row(d, mu, c6);
#pragma unroll
    for (int j = 0; j < 3; ++j) tm[t * 3 + j] = mu[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) tc[t * 6 + j] = c6[j];
  }
  __syncthreads();
  run_copy(m.means + base * 3, tm, rows * 3, t);
  run_copy(m.cov_triu + base * 6, tc, rows * 6, t);
}

}  // namespace

extern "C" size_t s3a_reanchor_workspace_bytes(int32_t n_kf) {
  if (n_kf <= 0) return 0;
  return (size_t)n_kf * kDelta * sizeof(double);
}

extern "C" void s3a_set_path(int path) { g_path.store(path == 1 ? 1 : 0); }

extern "C" int s3a_map_reanchor(const s3w_map* map, float* anchor, const float* poses,
                                int32_t n_kf, int64_t* moved, int64_t* held, void* workspace,
                                size_t workspace_bytes, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n_kf > 0, "s3a_map_reanchor: n_kf <= 0");
  S3_REQUIRE(n_kf <= (1 << 24), "s3a_map_reanchor: n_kf too large");
  S3_REQUIRE(workspace && workspace_bytes >= s3a_reanchor_workspace_bytes(n_kf),
             "s3a_map_reanchor: workspace too small");
  S3_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
             "s3a_map_reanchor: workspace must be 8-byte aligned");
  S3_REQUIRE(map && map->means && map->cov_triu && map->kf_id && map->n && map->cap > 0,
             "s3a_map_reanchor: bad map");
  S3_REQUIRE(map->cap < ((int64_t)1 << 31) * kT, "s3a_map_reanchor: capacity too large");
  S3_REQUIRE(anchor && poses, "s3a_map_reanchor: null pose table");
  const int path = g_path.load();
  const uintptr_t align = path == 1 ? 15 : 7;
  S3_REQUIRE((reinterpret_cast<uintptr_t>(map->means) & align) == 0 &&
                 (reinterpret_cast<uintptr_t>(map->cov_triu) & align) == 0,
             "s3a_map_reanchor: means and cov_triu must be %d-byte aligned", (int)align + 1);
  hipStream_t st = s3::as_stream(stream);
  auto* mv = reinterpret_cast<ull*>(moved);
  auto* hd = reinterpret_cast<ull*>(held);
  if (mv) S3_HIP(hipMemsetAsync(mv, 0, sizeof(ull), st));
  if (hd) S3_HIP(hipMemsetAsync(hd, 0, sizeof(ull), st));
  double* delta = static_cast<double*>(workspace);
  k_reanchor_delta<<<(unsigned)s3::cdiv(n_kf, kT), kT, 0, st>>>(anchor, poses, n_kf, delta, hd);
  S3_LAUNCH_CHECK();
  const unsigned blocks = (unsigned)s3::cdiv(map->cap, kT);
  if (path == 1)
    k_reanchor_rows_lds<<<blocks, kT, 0, st>>>(*map, n_kf, delta, mv);
  else
    k_reanchor_rows<<<blocks, kT, 0, st>>>(*map, n_kf, delta, mv);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
