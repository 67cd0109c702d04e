// Splat optimiser (include/s3o.h s3o_activate / s3o_adam_step); the
// per-Gaussian arithmetic is splat_opt_math.hpp.
//
// k_splat_activate  one Gaussian per thread: its 14-float row in, its entries
//                   of the five structure-of-arrays rasterizer inputs out.
// k_splat_adam      one Gaussian per thread: radii[i] first (a culled row
//                   ends there: nothing else loaded, nothing stored), then
//                   the 14 gradients, the row and its two moment rows in,
//                   the three rows out.
//
// The rows of rows14, exp_avg and exp_avg_sq are 56 bytes, a multiple of 8
// and not of 16: each thread moves its own row as seven 8-byte accesses.  A
// wave's seven accesses together cover its 3,584 contiguous bytes exactly
// once, so no byte is fetched from memory twice; each single instruction
// touches 8 of every 56 bytes.  The alternative, staging a workgroup's 256
// rows through LDS as one contiguous float4 run (k_map_to_splats), was not
// built: it loads and stores every row of the run, the culled ones included,
// which is what the sparse step exists to avoid.
#include "arg_check.hpp"
#include "common.hpp"
#include "s3o.h"
#include "splat_opt_math.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kRow = s3o::kRow;
// a grid has at most 2^31 - 1 workgroups
constexpr int64_t kMaxRows = (((int64_t)1 << 31) - 1) * kThreads;

__global__ void __launch_bounds__(kThreads)
k_splat_activate(const float* __restrict__ rows14, int64_t n, float s,
                 float* __restrict__ means3D, float* __restrict__ shs,
                 float* __restrict__ opacities, float* __restrict__ scales,
                 float* __restrict__ rotations) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float r[kRow];
  s3w::load_row(rows14, i, r);
  float mean[3], sh[3], op, sc[3], q[4];
  s3o::activate(r, s, mean, sh, op, sc, q);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    means3D[i * 3 + k] = mean[k];
    shs[i * 3 + k] = sh[k];
    scales[i * 3 + k] = sc[k];
  }
  opacities[i] = op;
  reinterpret_cast<float4*>(rotations)[i] = make_float4(q[0], q[1], q[2], q[3]);
}

__global__ void __launch_bounds__(kThreads)
k_splat_adam(float* __restrict__ rows14, float* __restrict__ exp_avg,
             float* __restrict__ exp_avg_sq, int64_t n, const float* __restrict__ d_means3D,
             const float* __restrict__ d_shs, const float* __restrict__ d_opacities,
             const float* __restrict__ d_scales, const float* __restrict__ d_rotations,
             const int32_t* __restrict__ radii, s3o_adam hp, int32_t* __restrict__ skipped) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  if (radii && radii[i] <= 0) return;
  float dmean[3], dsh[3], dsc[3], dq[4];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dmean[k] = d_means3D[i * 3 + k];
    dsh[k] = d_shs[i * 3 + k];
    dsc[k] = d_scales[i * 3 + k];
  }
  const float dop = d_opacities[i];
  const float4 d4 = reinterpret_cast<const float4*>(d_rotations)[i];
  dq[0] = d4.x; dq[1] = d4.y; dq[2] = d4.z; dq[3] = d4.w;
  if (!s3o::all_finite(dmean, dsh, dop, dsc, dq)) {
    if (skipped) atomicAdd(skipped, 1);
    return;
  }
  float r[kRow], m[kRow], v[kRow];
  s3w::load_row(rows14, i, r);
  s3w::load_row(exp_avg, i, m);
  s3w::load_row(exp_avg_sq, i, v);
  s3o::adam_row(r, m, v, hp.render_scale, dmean, dsh, dop, dsc, dq, hp.lr, hp.beta1, hp.beta2,
                hp.eps, hp.bias1, hp.bias2_sqrt);
  s3w::store_row(rows14, i, r);
  s3w::store_row(exp_avg, i, m);
  s3w::store_row(exp_avg_sq, i, v);
}

}  // namespace

extern "C" int s3o_activate(const float* rows14, int64_t n, float render_scale, float* means3D,
                            float* shs, float* opacities, float* scales, float* rotations,
                            void* stream) {
  s3::clear_error();
  S3_REQUIRE(n >= 0, "s3o_activate: n < 0");
  S3_REQUIRE(n <= kMaxRows, "s3o_activate: n too large");
  S3_REQUIRE(render_scale > 0.0f && render_scale <= 3.402823466e+38f,
             "s3o_activate: render_scale must be > 0 and finite");
  if (n == 0) return S3_OK;
  S3_REQUIRE(rows14 && means3D && shs && opacities && scales && rotations,
             "s3o_activate: null argument");
  S3_REQUIRE(s3::aligned(rows14, 8), "s3o_activate: rows14 must be 8-byte aligned");
  S3_REQUIRE(s3::aligned(rotations, 16), "s3o_activate: rotations must be 16-byte aligned");
  k_splat_activate<<<(unsigned)s3::cdiv(n, kThreads), kThreads, 0, s3::as_stream(stream)>>>(
      rows14, n, render_scale, means3D, shs, opacities, scales, rotations);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" int s3o_adam_step(float* rows14, float* exp_avg, float* exp_avg_sq, int64_t n,
                             const float* d_means3D, const float* d_shs,
                             const float* d_opacities, const float* d_scales,
                             const float* d_rotations, const int32_t* radii, const s3o_adam* hp,
                             int32_t* skipped, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n >= 0, "s3o_adam_step: n < 0");
  S3_REQUIRE(n <= kMaxRows, "s3o_adam_step: n too large");
  S3_REQUIRE(hp, "s3o_adam_step: null hyperparameters");
  for (int k = 0; k < s3o::kGroups; ++k)
    S3_REQUIRE(hp->lr[k] >= 0.0f && hp->lr[k] <= 3.402823466e+38f,
               "s3o_adam_step: lr[%d] must be >= 0 and finite", k);
  S3_REQUIRE(hp->beta1 >= 0.0f && hp->beta1 < 1.0f, "s3o_adam_step: beta1 must be in [0, 1)");
  S3_REQUIRE(hp->beta2 >= 0.0f && hp->beta2 < 1.0f, "s3o_adam_step: beta2 must be in [0, 1)");
  S3_REQUIRE(hp->eps > 0.0f && hp->eps <= 3.402823466e+38f,
             "s3o_adam_step: eps must be > 0 and finite");
  S3_REQUIRE(hp->bias1 > 0.0f && hp->bias1 <= 1.0f, "s3o_adam_step: bias1 must be in (0, 1]");
  S3_REQUIRE(hp->bias2_sqrt > 0.0f && hp->bias2_sqrt <= 1.0f,
             "s3o_adam_step: bias2_sqrt must be in (0, 1]");
  S3_REQUIRE(hp->render_scale > 0.0f && hp->render_scale <= 3.402823466e+38f,
             "s3o_adam_step: render_scale must be > 0 and finite");
  if (n == 0) return S3_OK;
  S3_REQUIRE(rows14 && exp_avg && exp_avg_sq, "s3o_adam_step: null parameter or moment rows");
  S3_REQUIRE(d_means3D && d_shs && d_opacities && d_scales && d_rotations,
             "s3o_adam_step: null gradient");
  S3_REQUIRE(s3::aligned(rows14, 8) && s3::aligned(exp_avg, 8) && s3::aligned(exp_avg_sq, 8),
             "s3o_adam_step: rows14, exp_avg and exp_avg_sq must be 8-byte aligned");
  S3_REQUIRE(s3::aligned(d_rotations, 16), "s3o_adam_step: d_rotations must be 16-byte aligned");
  k_splat_adam<<<(unsigned)s3::cdiv(n, kThreads), kThreads, 0, s3::as_stream(stream)>>>(
      rows14, exp_avg, exp_avg_sq, n, d_means3D, d_shs, d_opacities, d_scales, d_rotations,
      radii, *hp, skipped);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
