// Adaptive density control of the splat rows (include/s3d.h); the
// per-Gaussian arithmetic is splat_density_math.hpp.
//
// k_density_accumulate  one Gaussian per thread: radii[i] first (a culled row
//                       ends there), then dx, dy and the three statistics.
// k_density_classify    one Gaussian per thread: its row and statistics in,
//                       its decision code (one byte) out; per block the
//                       number of rows not pruned and of rows that grow.
// k_density_scan        exclusive scan of the two block counts (one
//                       workgroup, 1,024 blocks a trip), the totals, n_out
//                       and the pruned / denied counts.
// k_density_emit        one input row per thread: the stored code, a
//                       block-local scan of both flags, then
//                         offset = (alive before i) + min(growing before i, cap - B)
//                       and the row's one or two output rows, moment rows
//                       and origin entries.
// k_density_reset_opacity  one Gaussian per thread, the three opacity entries.
//
// The emit reads the stored code and does not recompute the decision: the
// statistics (12 B a row) and the two exps and the sigmoid are paid once.
// Rows are 56 bytes: seven 8-byte accesses per row, as in splat_opt.hip.
#include "arg_check.hpp"
#include "common.hpp"
#include "s3d.h"
#include "splat_density_math.hpp"
#include "wave_scan.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kRow = s3d::kRow;
constexpr int kScanThreads = 1024;
// origin holds a row index as int32
constexpr int64_t kMaxRows = ((int64_t)1 << 31) - 1;

// alive in the low half, growing in the high half: a block holds at most 256
// of either, so the packed sums of one block never carry across.
__device__ __forceinline__ uint32_t pack_flags(int code) {
  return (code != s3d::kPrune ? 1u : 0u) | (code >= s3d::kClone ? 0x10000u : 0u);
}

__global__ void __launch_bounds__(kThreads)
k_density_accumulate(const float* __restrict__ d_means2D, const int32_t* __restrict__ radii,
                     int64_t n, float* __restrict__ grad_accum, int32_t* __restrict__ denom,
                     int32_t* __restrict__ max_radii) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t rad = radii[i];
  if (rad <= 0) return;
  const float g = s3d::grad_norm2d(d_means2D[i * 3], d_means2D[i * 3 + 1]);
  if (!(g >= 0.0f)) return;
  grad_accum[i] += g;
  denom[i] += 1;
  const int32_t m = max_radii[i];
  max_radii[i] = rad > m ? rad : m;
}

__global__ void __launch_bounds__(kThreads)
k_density_classify(const float* __restrict__ rows14, int64_t n,
                   const float* __restrict__ grad_accum, const int32_t* __restrict__ denom,
                   const int32_t* __restrict__ max_radii, s3d::Params p,
                   uint8_t* __restrict__ codes, uint32_t* __restrict__ b_alive,
                   uint32_t* __restrict__ b_grow) {
  __shared__ uint32_t s_w[kThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t f = 0;
  if (i < n) {
    float r[kRow];
    s3w::load_row(rows14, i, r);
    const int code = s3d::decide(r, grad_accum[i], denom[i], max_radii[i], p);
    codes[i] = (uint8_t)code;
    f = pack_flags(code);
  }
  uint32_t tot = 0;
  s3::block_excl_add<kThreads>(f, s_w, &tot);
  if (threadIdx.x == 0) {
    b_alive[blockIdx.x] = tot & 0xffffu;
    b_grow[blockIdx.x] = tot >> 16;
  }
}

// Exclusive scans of b_alive and b_grow in place, the totals in
// b_alive[nblk] and b_grow[nblk]; n_out and counts (pruned, 0, 0, denied:
// the emit adds the granted clones and splits).
__global__ void __launch_bounds__(kScanThreads)
k_density_scan(uint32_t* __restrict__ b_alive, uint32_t* __restrict__ b_grow, int64_t nblk,
               int64_t n, int64_t cap, int64_t* __restrict__ n_out, int32_t* __restrict__ counts) {
  __shared__ uint32_t s_w[kScanThreads / 64];
  uint32_t carry_a = 0, carry_g = 0;
  for (int64_t c0 = 0; c0 < nblk; c0 += kScanThreads) {
    const int64_t c = c0 + threadIdx.x;
    const uint32_t a = c < nblk ? b_alive[c] : 0u;
    const uint32_t g = c < nblk ? b_grow[c] : 0u;
    uint32_t tot_a = 0, tot_g = 0;
    const uint32_t ea = s3::block_excl_add<kScanThreads>(a, s_w, &tot_a);
    const uint32_t eg = s3::block_excl_add<kScanThreads>(g, s_w, &tot_g);
    if (c < nblk) {
      b_alive[c] = carry_a + ea;
      b_grow[c] = carry_g + eg;
    }
    carry_a += tot_a;
    carry_g += tot_g;
  }
  if (threadIdx.x == 0) {
    b_alive[nblk] = carry_a;
    b_grow[nblk] = carry_g;
    const int64_t B = carry_a, G = carry_g;
    const int64_t budget = cap - B;
    const int64_t granted = G < budget ? G : budget;
    *n_out = B + granted;
    counts[0] = (int32_t)(n - B);
    counts[1] = 0;
    counts[2] = 0;
    counts[3] = (int32_t)(G - granted);
  }
}

__global__ void __launch_bounds__(kThreads)
k_density_emit(const float* __restrict__ rows14, const float* __restrict__ exp_avg,
               const float* __restrict__ exp_avg_sq, int64_t n,
               const uint8_t* __restrict__ codes, const uint32_t* __restrict__ b_alive,
               const uint32_t* __restrict__ b_grow, int64_t nblk, int64_t cap, uint64_t seed,
               uint32_t pass, float* __restrict__ out_rows, float* __restrict__ out_m,
               float* __restrict__ out_v, int32_t* __restrict__ origin,
               int32_t* __restrict__ counts) {
  __shared__ uint32_t s_w[kThreads / 64];
  __shared__ uint32_t s_cnt[2];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
  const int code = i < n ? (int)codes[i] : s3d::kPrune;
  const uint32_t f = pack_flags(code);
  const uint32_t ex = s3::block_excl_add<kThreads>(f, s_w, nullptr);  // both barriers: s_cnt is set
  if (code != s3d::kPrune) {
    const int64_t alive_before = (int64_t)b_alive[blockIdx.x] + (ex & 0xffffu);
    const int64_t grow_before = (int64_t)b_grow[blockIdx.x] + (ex >> 16);
    const int64_t budget = cap - (int64_t)b_alive[nblk];
    const int64_t off = alive_before + (grow_before < budget ? grow_before : budget);
    const bool grows = code >= s3d::kClone && grow_before < budget;
    float r[kRow], m[kRow];
    s3w::load_row(rows14, i, r);
    if (grows && code == s3d::kSplit) {
      float c[kRow];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        s3d::split_child(r, i, pass, (uint32_t)k, seed, c);
        s3w::store_row(out_rows, off + k, c);
        s3w::zero_row(out_m, off + k);
        s3w::zero_row(out_v, off + k);
        origin[off + k] = ~(int32_t)i;
      }
      atomicAdd(&s_cnt[1], 1u);
    } else {
      s3w::store_row(out_rows, off, r);
      s3w::load_row(exp_avg, i, m);
      s3w::store_row(out_m, off, m);
      s3w::load_row(exp_avg_sq, i, m);
      s3w::store_row(out_v, off, m);
      origin[off] = (int32_t)i;
      if (grows) {
        s3w::store_row(out_rows, off + 1, r);
        s3w::zero_row(out_m, off + 1);
        s3w::zero_row(out_v, off + 1);
        origin[off + 1] = ~(int32_t)i;
        atomicAdd(&s_cnt[0], 1u);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x])
    atomicAdd(&counts[1 + threadIdx.x], (int32_t)s_cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(kThreads)
k_density_reset_opacity(float* __restrict__ rows14, float* __restrict__ exp_avg,
                        float* __restrict__ exp_avg_sq, int64_t n, float logit_cap) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float l = rows14[i * kRow + 6];
  if (l > logit_cap) rows14[i * kRow + 6] = logit_cap;   // a NaN logit stays, as torch.minimum
  exp_avg[i * kRow + 6] = 0.0f;
  exp_avg_sq[i * kRow + 6] = 0.0f;
}

struct Workspace {
  uint8_t* codes;
  uint32_t *b_alive, *b_grow;
  size_t bytes;
};

Workspace carve(void* base, int64_t n) {
  const int64_t nblk = s3::cdiv(n, kThreads);
  const size_t codes = ((size_t)n + 15) & ~(size_t)15;
  Workspace w;
  w.codes = static_cast<uint8_t*>(base);
  w.b_alive = reinterpret_cast<uint32_t*>(w.codes + codes);
  w.b_grow = w.b_alive + (nblk + 1);
  w.bytes = codes + 2 * (size_t)(nblk + 1) * sizeof(uint32_t);
  return w;
}

}  // namespace

extern "C" size_t s3d_workspace_bytes(int64_t n) {
  if (n <= 0) return 16;
  return carve(nullptr, n).bytes;
}

extern "C" int s3d_accumulate(const float* d_means2D, const int32_t* radii, int64_t n,
                              float* grad_accum, int32_t* denom, int32_t* max_radii,
                              void* stream) {
  s3::clear_error();
  S3_REQUIRE(n >= 0, "s3d_accumulate: n < 0");
  S3_REQUIRE(n <= kMaxRows, "s3d_accumulate: n too large");
  if (n == 0) return S3_OK;
  S3_REQUIRE(d_means2D && radii && grad_accum && denom && max_radii,
             "s3d_accumulate: null argument");
  k_density_accumulate<<<(unsigned)s3::cdiv(n, kThreads), kThreads, 0, s3::as_stream(stream)>>>(
      d_means2D, radii, n, grad_accum, denom, max_radii);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" int s3d_densify(const float* rows14, const float* exp_avg, const float* exp_avg_sq,
                           int64_t n, const float* grad_accum, const int32_t* denom,
                           const int32_t* max_radii, const s3d_params* params, int64_t cap,
                           float* out_rows, float* out_exp_avg, float* out_exp_avg_sq,
                           int32_t* origin, int64_t* n_out, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n >= 0, "s3d_densify: n < 0");
  S3_REQUIRE(n <= kMaxRows, "s3d_densify: n too large");
  S3_REQUIRE(cap >= n, "s3d_densify: cap < n");
  S3_REQUIRE(params, "s3d_densify: null params");
  S3_REQUIRE(params->grad_threshold == params->grad_threshold &&
                 params->split_scale == params->split_scale &&
                 params->min_opacity == params->min_opacity &&
                 params->max_scale == params->max_scale,
             "s3d_densify: a threshold is NaN");
  if (n == 0) return S3_OK;
  S3_REQUIRE(rows14 && exp_avg && exp_avg_sq, "s3d_densify: null parameter or moment rows");
  S3_REQUIRE(grad_accum && denom && max_radii, "s3d_densify: null statistics");
  S3_REQUIRE(out_rows && out_exp_avg && out_exp_avg_sq && origin && n_out && counts,
             "s3d_densify: null output");
  S3_REQUIRE(workspace, "s3d_densify: null workspace");
  const Workspace w = carve(workspace, n);
  if (workspace_bytes < w.bytes) {
    s3::set_error("s3d_densify: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
    return S3_ERR_WORKSPACE;
  }
  S3_REQUIRE(s3::aligned(workspace, 4), "s3d_densify: workspace must be 4-byte aligned");
  S3_REQUIRE(s3::aligned(rows14, 8) && s3::aligned(exp_avg, 8) && s3::aligned(exp_avg_sq, 8) &&
                 s3::aligned(out_rows, 8) && s3::aligned(out_exp_avg, 8) && s3::aligned(out_exp_avg_sq, 8),
             "s3d_densify: row arrays must be 8-byte aligned");
  const size_t in_b = (size_t)n * kRow * sizeof(float), out_b = (size_t)cap * kRow * sizeof(float);
  const float* ins[3] = {rows14, exp_avg, exp_avg_sq};
  float* outs[3] = {out_rows, out_exp_avg, out_exp_avg_sq};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b)
      S3_REQUIRE(!s3::overlap(outs[a], out_b, ins[b], in_b),
                 "s3d_densify: an output overlaps an input");
    for (int b = a + 1; b < 3; ++b)
      S3_REQUIRE(!s3::overlap(outs[a], out_b, outs[b], out_b), "s3d_densify: outputs overlap");
  }
  const int64_t nblk = s3::cdiv(n, kThreads);
  hipStream_t st = s3::as_stream(stream);
  const s3d::Params p = {params->grad_threshold, params->split_scale, params->min_opacity,
                         params->max_scale, params->max_screen_radius};
  k_density_classify<<<(unsigned)nblk, kThreads, 0, st>>>(rows14, n, grad_accum, denom, max_radii,
                                                          p, w.codes, w.b_alive, w.b_grow);
  S3_LAUNCH_CHECK();
  k_density_scan<<<1, kScanThreads, 0, st>>>(w.b_alive, w.b_grow, nblk, n, cap, n_out, counts);
  S3_LAUNCH_CHECK();
  k_density_emit<<<(unsigned)nblk, kThreads, 0, st>>>(
      rows14, exp_avg, exp_avg_sq, n, w.codes, w.b_alive, w.b_grow, nblk, cap, params->seed,
      params->pass, out_rows, out_exp_avg, out_exp_avg_sq, origin, counts);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" int s3d_reset_opacity(float* rows14, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 float logit_cap, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n >= 0, "s3d_reset_opacity: n < 0");
  S3_REQUIRE(n <= kMaxRows, "s3d_reset_opacity: n too large");
  S3_REQUIRE(logit_cap == logit_cap, "s3d_reset_opacity: logit_cap is NaN");
  if (n == 0) return S3_OK;
  S3_REQUIRE(rows14 && exp_avg && exp_avg_sq, "s3d_reset_opacity: null argument");
  k_density_reset_opacity<<<(unsigned)s3::cdiv(n, kThreads), kThreads, 0,
                            s3::as_stream(stream)>>>(rows14, exp_avg, exp_avg_sq, n, logit_cap);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
