// Co-visibility loss mask (include/s3c.h), written for gfx950.
//
// k_loss_mask_inv:  one thread per view: inverse(K_1) (adjugate) and
//                   inverse(c2w_2) (cofactors) in closed form in double, rounded
//                   to float32 into the workspace.
// k_loss_mask:      one thread per target pixel, a 32 x 8 pixel tile per
//                   256-lane workgroup, looping over the context views.  The
//                   matrices of a (b, view) pair are wave-uniform loads; the
//                   four depth_2 taps per context view are a coherent gather
//                   (neighbouring target pixels land on neighbouring context
//                   pixels) served by the caches, no LDS.
//
// The file is built with -ffp-contract=off: the float32 chain below is the
// reference's chain of einsums, each product and sum rounded on its own.
#include "common.hpp"
#include "s3c.h"

namespace {

constexpr int kTW = 32;
constexpr int kTH = 8;
constexpr int kThreads = kTW * kTH;
constexpr int kMaxDim = 1 << 15;

// inverse of a row-major 3 x 3 by its adjugate
__host__ __device__ inline void inverse3(const double* a, double* b) {
  const double c00 = a[4] * a[8] - a[5] * a[7];
  const double c01 = a[5] * a[6] - a[3] * a[8];
  const double c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  b[0] = c00 / det;
  b[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  b[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  b[3] = c01 / det;
  b[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  b[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  b[6] = c02 / det;
  b[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  b[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// inverse of a row-major 4 x 4 by cofactors, from the 2 x 2 minors of its
// upper (s) and lower (c) row pairs
__host__ __device__ inline void inverse4(const double* a, double* b) {
  const double s0 = a[0] * a[5] - a[4] * a[1];
  const double s1 = a[0] * a[6] - a[4] * a[2];
  const double s2 = a[0] * a[7] - a[4] * a[3];
  const double s3 = a[1] * a[6] - a[5] * a[2];
  const double s4 = a[1] * a[7] - a[5] * a[3];
  const double s5 = a[2] * a[7] - a[6] * a[3];
  const double c5 = a[10] * a[15] - a[14] * a[11];
  const double c4 = a[9] * a[15] - a[13] * a[11];
  const double c3 = a[9] * a[14] - a[13] * a[10];
  const double c2 = a[8] * a[15] - a[12] * a[11];
  const double c1 = a[8] * a[14] - a[12] * a[10];
  const double c0 = a[8] * a[13] - a[12] * a[9];
  const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  b[0] = (a[5] * c5 - a[6] * c4 + a[7] * c3) / det;
  b[1] = (-a[1] * c5 + a[2] * c4 - a[3] * c3) / det;
  b[2] = (a[13] * s5 - a[14] * s4 + a[15] * s3) / det;
  b[3] = (-a[9] * s5 + a[10] * s4 - a[11] * s3) / det;
  b[4] = (-a[4] * c5 + a[6] * c2 - a[7] * c1) / det;
  b[5] = (a[0] * c5 - a[2] * c2 + a[3] * c1) / det;
  b[6] = (-a[12] * s5 + a[14] * s2 - a[15] * s1) / det;
  b[7] = (a[8] * s5 - a[10] * s2 + a[11] * s1) / det;
  b[8] = (a[4] * c4 - a[5] * c2 + a[7] * c0) / det;
  b[9] = (-a[0] * c4 + a[1] * c2 - a[3] * c0) / det;
  b[10] = (a[12] * s4 - a[13] * s2 + a[15] * s0) / det;
  b[11] = (-a[8] * s4 + a[9] * s2 - a[11] * s0) / det;
  b[12] = (-a[4] * c3 + a[5] * c1 - a[6] * c0) / det;
  b[13] = (a[0] * c3 - a[1] * c1 + a[2] * c0) / det;
  b[14] = (-a[12] * s3 + a[13] * s1 - a[14] * s0) / det;
  b[15] = (a[8] * s3 - a[9] * s1 + a[10] * s0) / det;
}

template <int N>
__host__ __device__ inline void invert_f32(const float* src, float* dst) {
  double a[N * N], b[N * N];
#pragma unroll
  for (int k = 0; k < N * N; ++k) a[k] = (double)src[k];
  if (N == 3) inverse3(a, b);
  else inverse4(a, b);
#pragma unroll
  for (int k = 0; k < N * N; ++k) dst[k] = (float)b[k];
}

// n1 = B V1 intrinsics, then n2 = B V2 poses
__global__ __launch_bounds__(64) void k_loss_mask_inv(const float* __restrict__ K_1,
                                                      const float* __restrict__ c2w_2, int n1,
                                                      int n2, float* __restrict__ Kinv_1,
                                                      float* __restrict__ w2c_2) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t < n1) invert_f32<3>(K_1 + (size_t)t * 9, Kinv_1 + (size_t)t * 9);
  else if (t < n1 + n2) invert_f32<4>(c2w_2 + (size_t)(t - n1) * 16, w2c_2 + (size_t)(t - n1) * 16);
}

// One tap of the zero-padded bilinear sample.  The bound check is in floating
// point, so a NaN, an infinity or a value beyond the int range never becomes
// an index: inside the branch 0 <= fx <= W - 1 and 0 <= fy <= H - 1 hold.
__host__ __device__ __forceinline__ float tap(const float* __restrict__ img, float fx, float fy,
                                              int H, int W) {
  if (fx >= 0.f && fx <= (float)(W - 1) && fy >= 0.f && fy <= (float)(H - 1))
    return img[(size_t)(int)fy * W + (int)fx];
  return 0.f;
}

// The S3C_COND_* bits of target pixel (x, y) with depth d.  Ki = inverse(K_1)
// and T1 = c2w_1 of its view; T2, K2, img: inverse(c2w_2), K_2 and depth_2 of
// the V2 context views of its batch entry.
__host__ __device__ __forceinline__ unsigned pixel_conditions(
    int x, int y, float d, const float* __restrict__ Ki, const float* __restrict__ T1,
    const float* __restrict__ T2, const float* __restrict__ K2, const float* __restrict__ img,
    int V2, int H, int W) {
  const float px = (float)x, py = (float)y;
  // cam = (Kinv (x, y, 1)) d
  float cam[3], world[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    cam[r] = (Ki[3 * r] * px + Ki[3 * r + 1] * py + Ki[3 * r + 2] * 1.f) * d;
  // world = c2w_1 (cam, 1)
#pragma unroll
  for (int r = 0; r < 3; ++r)
    world[r] = T1[4 * r] * cam[0] + T1[4 * r + 1] * cam[1] + T1[4 * r + 2] * cam[2] +
               T1[4 * r + 3] * 1.f;

  bool any_fr = false, any_md = false;
  const float fW = (float)W, fH = (float)H;
  for (int j = 0; j < V2; ++j, T2 += 16, K2 += 9, img += (size_t)H * W) {
    float cp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      cp[r] = T2[4 * r] * world[0] + T2[4 * r + 1] * world[1] + T2[4 * r + 2] * world[2] +
              T2[4 * r + 3] * 1.f;
    const float z = cp[2];
    const float nx = cp[0] / z, ny = cp[1] / z, nz = z / z;
    const float u = K2[0] * nx + K2[1] * ny + K2[2] * nz;
    const float v = K2[3] * nx + K2[4] * ny + K2[5] * nz;
    any_fr |= u > 0.f && u < fW && v > 0.f && v < fH;

    // bilinear sample at (u - 0.5, v - 0.5), zeros outside
    const float ix = u - 0.5f, iy = v - 0.5f;
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float wx1 = ix - x0, wy1 = iy - y0;
    const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    // a non-finite coordinate reads no tap (tap() returns the padding's 0)
    // and has NaN weights, so s is NaN and md false, as in the reference
    float s = tap(img, x0, y0, H, W) * (wy0 * wx0);
    s = s + tap(img, x0 + 1.f, y0, H, W) * (wy0 * wx1);
    s = s + tap(img, x0, y0 + 1.f, H, W) * (wy1 * wx0);
    s = s + tap(img, x0 + 1.f, y0 + 1.f, H, W) * (wy1 * wx1);
    any_md |= z == s || fabsf(z - s) <= 0.1f + 1e-5f * fabsf(s);
  }
  return (any_fr ? S3C_COND_FRUSTUM : 0u) | (d > 1e-6f ? S3C_COND_DEPTH : 0u) |
         (any_md ? S3C_COND_MATCH : 0u);
}

__global__ __launch_bounds__(kThreads) void k_loss_mask(
    const float* __restrict__ depth_1, const float* __restrict__ Kinv_1,
    const float* __restrict__ c2w_1, const float* __restrict__ depth_2,
    const float* __restrict__ K_2, const float* __restrict__ w2c_2, int V1, int V2, int H, int W,
    uint8_t* __restrict__ mask, float* __restrict__ mask_f32, uint8_t* __restrict__ conditions) {
  const int x = (int)blockIdx.x * kTW + (int)(threadIdx.x % kTW);
  const int y = (int)blockIdx.y * kTH + (int)(threadIdx.x / kTW);
  const int bi = (int)blockIdx.z;   // b * V1 + i
  if (x >= W || y >= H) return;
  const size_t pix = ((size_t)bi * H + y) * W + x;
  const size_t bj = (size_t)(bi / V1) * V2;   // first context view of this batch entry
  const unsigned c = pixel_conditions(x, y, depth_1[pix], Kinv_1 + (size_t)bi * 9,
                                      c2w_1 + (size_t)bi * 16, w2c_2 + bj * 16, K_2 + bj * 9,
                                      depth_2 + bj * H * W, V2, H, W);
  const bool m = c == (S3C_COND_FRUSTUM | S3C_COND_DEPTH | S3C_COND_MATCH);
  mask[pix] = (uint8_t)m;
  if (mask_f32) mask_f32[pix] = m ? 1.f : 0.f;
  if (conditions) conditions[pix] = (uint8_t)c;
}

size_t inv_floats(int B, int V1, int V2) { return (size_t)B * V1 * 9 + (size_t)B * V2 * 16; }

}  // namespace

extern "C" {

size_t s3c_loss_mask_workspace_bytes(int B, int V1, int V2) {
  if (B <= 0 || V1 <= 0 || V2 <= 0) return 0;
  return inv_floats(B, V1, V2) * sizeof(float);
}

int s3c_loss_mask(const float* depth_1, const float* K_1, const float* c2w_1,
                  const float* depth_2, const float* K_2, const float* c2w_2,
                  int B, int V1, int V2, int H, int W,
                  uint8_t* mask, float* mask_f32, uint8_t* conditions,
                  void* workspace, void* stream) {
  s3::clear_error();
  S3_REQUIRE(B > 0 && V1 > 0 && V2 > 0 && (int64_t)B * V1 <= 65535 && (int64_t)B * V2 <= 65535,
             "s3c_loss_mask: B = %d, V1 = %d, V2 = %d, expected B V1 and B V2 in 1 .. 65535", B,
             V1, V2);
  S3_REQUIRE(H > 0 && W > 0 && H <= kMaxDim && W <= kMaxDim,
             "s3c_loss_mask: image %d x %d, expected 1 .. %d per side", H, W, kMaxDim);
  S3_REQUIRE(depth_1 && K_1 && c2w_1 && depth_2 && K_2 && c2w_2 && mask,
             "s3c_loss_mask: inputs and mask must not be NULL");
  if (!workspace) {
    s3::set_error("s3c_loss_mask: workspace is NULL (%zu bytes needed)",
                  s3c_loss_mask_workspace_bytes(B, V1, V2));
    return S3_ERR_WORKSPACE;
  }
  hipStream_t st = s3::as_stream(stream);
  float* Kinv_1 = static_cast<float*>(workspace);
  float* w2c_2 = Kinv_1 + (size_t)B * V1 * 9;
  const int n1 = B * V1, n2 = B * V2;
  hipLaunchKernelGGL(k_loss_mask_inv, dim3((unsigned)s3::cdiv(n1 + n2, 64)), dim3(64), 0, st, K_1,
                     c2w_2, n1, n2, Kinv_1, w2c_2);
  S3_LAUNCH_CHECK();
  const dim3 grid((unsigned)s3::cdiv(W, kTW), (unsigned)s3::cdiv(H, kTH), (unsigned)n1);
  hipLaunchKernelGGL(k_loss_mask, grid, dim3(kThreads), 0, st, depth_1, Kinv_1, c2w_1, depth_2,
                     K_2, w2c_2, V1, V2, H, W, mask, mask_f32, conditions);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

}  // extern "C"
