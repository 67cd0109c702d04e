// Pose gradient and pose step (include/s3x.h); the arithmetic is
// pose_grad_math.hpp.
//
// k_pose_grad      a workgroup of 256 threads owns kRowsPerBlock = 2,048
//                  consecutive rows, eight per thread, row j * 256 + thread of
//                  the block in trip j (a wave's loads are contiguous).  A
//                  thread reads radii[i] first: a culled row ends there.  The
//                  six double sums go through a wave butterfly, then through
//                  LDS across the four waves in wave order, and thread k < 6
//                  writes the workgroup's partial k.  Eight rows per thread
//                  keep the partials of the 8.39 M-row map to 4,096 (196 KB),
//                  16 trips of the second stage, and still give every CU 16
//                  workgroups.
// k_pose_grad_sum  one workgroup: thread t sums partials t, t + 256, ... in
//                  that order, then the same wave + LDS reduction; writes
//                  out[6].  With no partial at all it writes six zeros.
// No floating-point atomic anywhere: the result is a pure function of the
// inputs and n.  The skipped counter is an integer atomic.
// k_pose_step      one thread (s3x::pose_step, s3x::pose_camera).
#include "arg_check.hpp"
#include "common.hpp"
#include "pose_grad_math.hpp"
#include "s3x.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerThread = 8;
constexpr int64_t kRowsPerBlock = (int64_t)kThreads * kRowsPerThread;
// a grid has at most 2^31 - 1 workgroups
constexpr int64_t kMaxRows = (((int64_t)1 << 31) - 1) * kRowsPerBlock;

// Workgroup sum of six per-thread doubles, in a fixed order; the totals are
// returned in threads 0..5 (thread k holds sum k), other threads return 0.
__device__ __forceinline__ double block_sum6(const double (&acc)[6], double (&lds)[kWaves][6]) {
  double v[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    v[k] = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] = v[k] + __shfl_xor(v[k], o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) lds[wave][k] = v[k];
  }
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x < 6) {
    total = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) total = total + lds[w][threadIdx.x];
  }
  return total;
}

template <bool kCov>
__global__ void __launch_bounds__(kThreads)
k_pose_grad(const float* __restrict__ viewmatrix, const float* __restrict__ means3D,
            const float* __restrict__ d_means3D, const float* __restrict__ shape,
            const float* __restrict__ d_shape, const int32_t* __restrict__ radii, int64_t n,
            double* __restrict__ partials, int32_t* __restrict__ skipped) {
  __shared__ double lds[kWaves][6];
  s3x::Cam cam;
  s3x::cam_from_view(viewmatrix, cam);   // uniform: scalar loads, wave-uniform arithmetic
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t base = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x;
  int bad = 0;
#pragma unroll 2
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int64_t i = base + (int64_t)j * kThreads;
    if (i >= n) break;
    if (radii && radii[i] <= 0) continue;
    const float mu[3] = {means3D[i * 3], means3D[i * 3 + 1], means3D[i * 3 + 2]};
    const float dmu[3] = {d_means3D[i * 3], d_means3D[i * 3 + 1], d_means3D[i * 3 + 2]};
    bool ok;
    if (kCov) {
      const float2* s2 = reinterpret_cast<const float2*>(shape + i * 6);
      const float2* d2 = reinterpret_cast<const float2*>(d_shape + i * 6);
      const float2 s0 = s2[0], s1 = s2[1], s2v = s2[2], d0 = d2[0], d1 = d2[1], d2v = d2[2];
      const float cov[6] = {s0.x, s0.y, s1.x, s1.y, s2v.x, s2v.y};
      const float dcov[6] = {d0.x, d0.y, d1.x, d1.y, d2v.x, d2v.y};
      ok = s3x::sub_row_cov(cam, mu, dmu, cov, dcov, acc);
    } else {
      const float4 q4 = reinterpret_cast<const float4*>(shape)[i];
      const float4 d4 = reinterpret_cast<const float4*>(d_shape)[i];
      const float q[4] = {q4.x, q4.y, q4.z, q4.w};
      const float dq[4] = {d4.x, d4.y, d4.z, d4.w};
      ok = s3x::sub_row_rot(cam, mu, dmu, q, dq, acc);
    }
    if (!ok) ++bad;
  }
  if (bad && skipped) atomicAdd(skipped, bad);
  const double total = block_sum6(acc, lds);
  if (threadIdx.x < 6) partials[(int64_t)blockIdx.x * 6 + threadIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads)
k_pose_grad_sum(const double* __restrict__ partials, int64_t nblocks, double* __restrict__ out) {
  __shared__ double lds[kWaves][6];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t p = threadIdx.x; p < nblocks; p += kThreads) {
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = acc[k] + partials[p * 6 + k];
  }
  const double total = block_sum6(acc, lds);
  if (threadIdx.x < 6) out[threadIdx.x] = total;
}

__global__ void k_pose_step(double* __restrict__ T_WC, double* __restrict__ exp_avg,
                            double* __restrict__ exp_avg_sq, const double* __restrict__ grad,
                            s3x::PoseAdam hp, const float* __restrict__ proj_t,
                            float* __restrict__ view, float* __restrict__ full,
                            float* __restrict__ campos) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double T[16];
  for (int k = 0; k < 16; ++k) T[k] = T_WC[k];
  if (grad) {
    double m[6], v[6], g[6];
    for (int k = 0; k < 6; ++k) {
      m[k] = exp_avg[k];
      v[k] = exp_avg_sq[k];
      g[k] = grad[k];
    }
    if (s3x::pose_step(T, m, v, g, hp)) {
      for (int k = 0; k < 16; ++k) T_WC[k] = T[k];
      for (int k = 0; k < 6; ++k) {
        exp_avg[k] = m[k];
        exp_avg_sq[k] = v[k];
      }
    }
  }
  float fv[16], ff[16], fc[3];
  s3x::pose_camera(T, hp.render_scale, proj_t, fv, ff, fc);
  for (int k = 0; k < 16; ++k) {
    view[k] = fv[k];
    full[k] = ff[k];
  }
  for (int k = 0; k < 3; ++k) campos[k] = fc[k];
}

inline bool finite_nonneg(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }

}  // namespace

extern "C" size_t s3x_pose_grad_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  const int64_t blocks = s3::cdiv(n, kRowsPerBlock);
  return (size_t)(blocks > 0 ? blocks : 1) * 6 * sizeof(double);
}

extern "C" int s3x_pose_grad(const float* viewmatrix, const float* means3D,
                             const float* d_means3D, const float* cov3D, const float* d_cov3D,
                             const float* rotations, const float* d_rotations,
                             const int32_t* radii, int64_t n, double* out, int32_t* skipped,
                             void* workspace, size_t workspace_bytes, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n >= 0, "s3x_pose_grad: n < 0");
  S3_REQUIRE(n <= kMaxRows, "s3x_pose_grad: n too large");
  S3_REQUIRE(out, "s3x_pose_grad: null out");
  S3_REQUIRE(s3::aligned(out, 8), "s3x_pose_grad: out must be 8-byte aligned");
  const bool has_cov = cov3D || d_cov3D, has_rot = rotations || d_rotations;
  S3_REQUIRE(has_cov != has_rot,
             "s3x_pose_grad: give either cov3D and d_cov3D or rotations and d_rotations");
  if (has_cov)
    S3_REQUIRE(cov3D && d_cov3D, "s3x_pose_grad: cov3D and d_cov3D go together");
  else
    S3_REQUIRE(rotations && d_rotations, "s3x_pose_grad: rotations and d_rotations go together");
  hipStream_t st = s3::as_stream(stream);
  const int64_t blocks = s3::cdiv(n, kRowsPerBlock);
  if (n > 0) {
    S3_REQUIRE(viewmatrix && means3D && d_means3D, "s3x_pose_grad: null argument");
    S3_REQUIRE(workspace && workspace_bytes >= s3x_pose_grad_workspace_bytes(n),
               "s3x_pose_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
               s3x_pose_grad_workspace_bytes(n));
    S3_REQUIRE(s3::aligned(workspace, 8), "s3x_pose_grad: workspace must be 8-byte aligned");
    double* partials = static_cast<double*>(workspace);
    if (has_cov) {
      S3_REQUIRE(s3::aligned(cov3D, 8) && s3::aligned(d_cov3D, 8),
                 "s3x_pose_grad: cov3D and d_cov3D must be 8-byte aligned");
      k_pose_grad<true><<<(unsigned)blocks, kThreads, 0, st>>>(
          viewmatrix, means3D, d_means3D, cov3D, d_cov3D, radii, n, partials, skipped);
    } else {
      S3_REQUIRE(s3::aligned(rotations, 16) && s3::aligned(d_rotations, 16),
                 "s3x_pose_grad: rotations and d_rotations must be 16-byte aligned");
      k_pose_grad<false><<<(unsigned)blocks, kThreads, 0, st>>>(
          viewmatrix, means3D, d_means3D, rotations, d_rotations, radii, n, partials, skipped);
    }
    S3_LAUNCH_CHECK();
  }
  k_pose_grad_sum<<<1, kThreads, 0, st>>>(static_cast<const double*>(workspace), blocks, out);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" int s3x_pose_step(double* T_WC, double* exp_avg, double* exp_avg_sq,
                             const double* grad, const s3x_pose_adam* hp, const float* proj_t,
                             float* viewmatrix, float* projmatrix, float* campos, void* stream) {
  s3::clear_error();
  S3_REQUIRE(hp, "s3x_pose_step: null hyperparameters");
  S3_REQUIRE(hp->render_scale > 0.0 && finite_nonneg(hp->render_scale),
             "s3x_pose_step: render_scale must be > 0 and finite");
  if (grad) {
    S3_REQUIRE(finite_nonneg(hp->lr_translation), "s3x_pose_step: lr_translation must be >= 0 and finite");
    S3_REQUIRE(finite_nonneg(hp->lr_rotation), "s3x_pose_step: lr_rotation must be >= 0 and finite");
    S3_REQUIRE(hp->beta1 >= 0.0 && hp->beta1 < 1.0, "s3x_pose_step: beta1 must be in [0, 1)");
    S3_REQUIRE(hp->beta2 >= 0.0 && hp->beta2 < 1.0, "s3x_pose_step: beta2 must be in [0, 1)");
    S3_REQUIRE(hp->eps > 0.0 && finite_nonneg(hp->eps), "s3x_pose_step: eps must be > 0 and finite");
    S3_REQUIRE(hp->bias1 > 0.0 && hp->bias1 <= 1.0, "s3x_pose_step: bias1 must be in (0, 1]");
    S3_REQUIRE(hp->bias2_sqrt > 0.0 && hp->bias2_sqrt <= 1.0,
               "s3x_pose_step: bias2_sqrt must be in (0, 1]");
    S3_REQUIRE(exp_avg && exp_avg_sq, "s3x_pose_step: null moments");
    S3_REQUIRE(s3::aligned(exp_avg, 8) && s3::aligned(exp_avg_sq, 8) && s3::aligned(grad, 8),
               "s3x_pose_step: grad and the moments must be 8-byte aligned");
  }
  S3_REQUIRE(T_WC && proj_t && viewmatrix && projmatrix && campos, "s3x_pose_step: null argument");
  S3_REQUIRE(s3::aligned(T_WC, 8), "s3x_pose_step: T_WC must be 8-byte aligned");
  const s3x::PoseAdam p{hp->lr_translation, hp->lr_rotation, hp->beta1, hp->beta2, hp->eps,
                        hp->bias1, hp->bias2_sqrt, hp->render_scale};
  k_pose_step<<<1, 64, 0, s3::as_stream(stream)>>>(T_WC, exp_avg, exp_avg_sq, grad, p, proj_t,
                                                   viewmatrix, projmatrix, campos);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
