// Photometric loss and render-quality sums (include/s3p.h), written for gfx950.
//
// Forward:  k_photo_fwd, one 256-lane workgroup per 32 x 16 tile of one
//           channel image.  The tile plus a 5-pixel halo of x and y (masked,
//           reflect-indexed) goes to LDS; the row pass filters the five
//           moments x, y, x^2, y^2, xy into LDS; the column pass, S, its three
//           partial derivatives and the five sums stay in registers.  Each
//           workgroup writes its five partial sums (double; lanes, then waves,
//           added in a fixed order); k_photo_sums adds a batch image's partials
//           in double in a fixed order.  No floating-point atomics.
// Backward: k_photo_bwd, same tiling.  The adjoint of the reflect-padded filter
//           folds the zero-extended correlation c of a map back at the borders,
//             Gt[q](j) = c(j) + c(-1 - j) + c(2n - 1 - j)   per axis,
//           i.e. input i reaches output j with weight
//             g[j - i] + g[(-1 - j) - i] + g[(2n - 1 - j) - i].
//           The taps are symmetric, so that weight is symmetric in (i, j): the
//           fold IS the reflect-padded filter, Gt = G.  The backward therefore
//           loads q = w * dS/d{ux, uxx, uxy} reflect-indexed and runs the
//           forward's two passes on it.
#include <cmath>

#include "common.hpp"
#include "s3p.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 32;            // tile width  (one output column per lane & 31)
constexpr int kTH = 16;            // tile height (two output rows per lane)
constexpr int kR = 5;              // window radius
constexpr int kTaps = 2 * kR + 1;
constexpr int kHW = kTW + 2 * kR;  // tile + halo
constexpr int kHH = kTH + 2 * kR;
constexpr int kPitch = kHW + 1;
constexpr int kRows = kTH / (kThreads / kTW);   // output rows per lane
constexpr float kC1 = 0.01f * 0.01f;
constexpr float kC2 = 0.03f * 0.03f;
constexpr int kMaxDim = 1 << 15;

static_assert(kThreads % kTW == 0 && kTH % (kThreads / kTW) == 0, "tile / workgroup shape");

struct Taps {
  float g[kTaps];
};

struct Geo {
  int C, H, W;
  int tiles_x, tiles_y;
};

Taps window() {
  double w[kTaps], sum = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double d = k - kR;
    w[k] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += w[k];
  }
  Taps t;
  for (int k = 0; k < kTaps; ++k) t.g[k] = (float)(w[k] / sum);
  return t;
}

// scipy's `reflect`: -1-i left of the image, 2n-1-i right of it; -1 where that
// is no pixel (only beyond the halo of a ragged last tile, never read back).
__device__ __forceinline__ int reflect(int i, int n) {
  if (i < 0) i = -1 - i;
  else if (i >= n) i = 2 * n - 1 - i;
  return (i >= 0 && i < n) ? i : -1;
}

__global__ __launch_bounds__(kThreads) void k_photo_fwd(
    const float* __restrict__ pred, const float* __restrict__ target,
    const float* __restrict__ mask, Geo geo, Taps taps, float cn, float* __restrict__ smap,
    float* __restrict__ d_ux, float* __restrict__ d_uxx, float* __restrict__ d_uxy,
    double* __restrict__ partials) {
  __shared__ float sx[kHH][kPitch];
  __shared__ float sy[kHH][kPitch];
  __shared__ float hm[5][kHH][kTW];
  __shared__ double red[kThreads / 64][S3P_NSUMS];

  const int tid = threadIdx.x;
  const int H = geo.H, W = geo.W;
  const int bc = blockIdx.z, b = bc / geo.C;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const size_t plane = (size_t)H * W;
  const float* P = pred + (size_t)bc * plane;
  const float* T = target + (size_t)bc * plane;
  const float* M = mask ? mask + (size_t)b * plane : nullptr;

  for (int i = tid; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i - r * kHW;
    const int gy = reflect(y0 + r - kR, H), gx = reflect(x0 + c - kR, W);
    float xv = 0.f, yv = 0.f;
    if (gy >= 0 && gx >= 0) {
      const size_t idx = (size_t)gy * W + gx;
      xv = P[idx];
      yv = T[idx];
      if (M) {
        const float m = M[idx];
        xv *= m;
        yv *= m;
      }
    }
    sx[r][c] = xv;
    sy[r][c] = yv;
  }
  __syncthreads();

  // row pass
  for (int i = tid; i < kHH * kTW; i += kThreads) {
    const int r = i / kTW, c = i - r * kTW;
    float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float xv = sx[r][c + k], yv = sy[r][c + k], g = taps.g[k];
      ax += g * xv;
      ay += g * yv;
      axx += g * (xv * xv);
      ayy += g * (yv * yv);
      axy += g * (xv * yv);
    }
    hm[0][r][c] = ax;
    hm[1][r][c] = ay;
    hm[2][r][c] = axx;
    hm[3][r][c] = ayy;
    hm[4][r][c] = axy;
  }
  __syncthreads();

  // column pass, S, derivatives, sums
  const int c = tid & (kTW - 1);
  const int gx = x0 + c;
  float acc[S3P_NSUMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int r = (tid / kTW) + j * (kThreads / kTW);
    const int gy = y0 + r;
    if (gy < H && gx < W) {
      float ux = 0.f, uy = 0.f, uxx = 0.f, uyy = 0.f, uxy = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const float g = taps.g[k];
        ux += g * hm[0][r + k][c];
        uy += g * hm[1][r + k][c];
        uxx += g * hm[2][r + k][c];
        uyy += g * hm[3][r + k][c];
        uxy += g * hm[4][r + k][c];
      }
      const float vx = cn * (uxx - ux * ux);
      const float vy = cn * (uyy - uy * uy);
      const float vxy = cn * (uxy - ux * uy);
      const float A1 = 2.f * ux * uy + kC1;
      const float A2 = 2.f * vxy + kC2;
      const float B1 = ux * ux + uy * uy + kC1;
      const float B2 = vx + vy + kC2;
      const float D = B1 * B2;
      const float S = (A1 * A2) / D;

      const size_t idx = (size_t)gy * W + gx;
      const size_t o = (size_t)bc * plane + idx;
      if (smap) smap[o] = S;
      if (d_ux) {
        // S as a function of (ux, uxx, uxy) with uy, uyy fixed; vx and vxy
        // depend on ux
        d_ux[o] = 2.f * uy * (A2 - cn * A1) / D - 2.f * ux * S / B1 + 2.f * cn * ux * S / B2;
        d_uxx[o] = -(cn * S) / B2;
        d_uxy[o] = 2.f * cn * A1 / D;
      }
      const float m = M ? M[idx] : 1.f;
      const float d = sx[r + kR][c + kR] - sy[r + kR][c + kR];
      acc[S3P_SUM_SQ] += m * (d * d);
      acc[S3P_SUM_ABS] += m * fabsf(d);
      acc[S3P_SUM_MS] += m * S;
      if (bc - b * geo.C == 0) acc[S3P_SUM_M] += m;
      if (gy >= kR && gy < H - kR && gx >= kR && gx < W - kR) acc[S3P_SUM_CROP] += S;
    }
  }

  // lanes (xor butterfly), then the four waves in order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int s = 0; s < S3P_NSUMS; ++s) {
    double v = (double)acc[s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][s] = v;
  }
  __syncthreads();
  if (tid < S3P_NSUMS) {
    double v = red[0][tid];
    for (int w = 1; w < kThreads / 64; ++w) v += red[w][tid];
    const size_t tile = (size_t)blockIdx.y * geo.tiles_x + blockIdx.x;
    partials[((size_t)bc * geo.tiles_x * geo.tiles_y + tile) * S3P_NSUMS + tid] = v;
  }
}

// One workgroup per batch image: lane t adds partials t, t + 256, ... in
// order, then a fixed LDS tree.
__global__ __launch_bounds__(kThreads) void k_photo_sums(const double* __restrict__ partials,
                                                         int n, double* __restrict__ sums) {
  __shared__ double red[kThreads][S3P_NSUMS];
  const int tid = threadIdx.x;
  const double* p = partials + (size_t)blockIdx.x * n * S3P_NSUMS;
  double acc[S3P_NSUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += kThreads)
#pragma unroll
    for (int s = 0; s < S3P_NSUMS; ++s) acc[s] += p[(size_t)i * S3P_NSUMS + s];
#pragma unroll
  for (int s = 0; s < S3P_NSUMS; ++s) red[tid][s] = acc[s];
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int s = 0; s < S3P_NSUMS; ++s) red[tid][s] += red[tid + o][s];
    __syncthreads();
  }
  if (tid < S3P_NSUMS) sums[(size_t)blockIdx.x * S3P_NSUMS + tid] = red[0][tid];
}

__global__ __launch_bounds__(kThreads) void k_photo_bwd(
    const float* __restrict__ pred, const float* __restrict__ target,
    const float* __restrict__ mask, const float* __restrict__ d_ux,
    const float* __restrict__ d_uxx, const float* __restrict__ d_uxy,
    const float* __restrict__ wmap, const float* __restrict__ coef, Geo geo, Taps taps,
    float* __restrict__ grad) {
  __shared__ float q[3][kHH][kPitch];
  __shared__ float hq[3][kHH][kTW];

  const int tid = threadIdx.x;
  const int H = geo.H, W = geo.W;
  const int bc = blockIdx.z, b = bc / geo.C;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const size_t plane = (size_t)H * W;
  const size_t base = (size_t)bc * plane;
  const float* M = mask ? mask + (size_t)b * plane : nullptr;
  const float ca = coef[b * 4 + 0], cb = coef[b * 4 + 1];
  const float c_ms = coef[b * 4 + 2], c_crop = coef[b * 4 + 3];

  // q = w dS/d{ux, uxx, uxy}, reflect-indexed like the forward's inputs
  for (int i = tid; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i - r * kHW;
    const int gy = reflect(y0 + r - kR, H), gx = reflect(x0 + c - kR, W);
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;
    if (gy >= 0 && gx >= 0) {
      const size_t idx = (size_t)gy * W + gx;
      float w = c_ms * (M ? M[idx] : 1.f);
      if (gy >= kR && gy < H - kR && gx >= kR && gx < W - kR) w += c_crop;
      if (wmap) w += wmap[base + idx];
      q0 = w * d_ux[base + idx];
      q1 = w * d_uxx[base + idx];
      q2 = w * d_uxy[base + idx];
    }
    q[0][r][c] = q0;
    q[1][r][c] = q1;
    q[2][r][c] = q2;
  }
  __syncthreads();

  // row pass
  for (int i = tid; i < kHH * kTW; i += kThreads) {
    const int r = i / kTW, c = i - r * kTW;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float g = taps.g[k];
      a0 += g * q[0][r][c + k];
      a1 += g * q[1][r][c + k];
      a2 += g * q[2][r][c + k];
    }
    hq[0][r][c] = a0;
    hq[1][r][c] = a1;
    hq[2][r][c] = a2;
  }
  __syncthreads();

  const int c = tid & (kTW - 1);
  const int gx = x0 + c;
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int r = (tid / kTW) + j * (kThreads / kTW);
    const int gy = y0 + r;
    if (gy < H && gx < W) {
      float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const float g = taps.g[k];
        t0 += g * hq[0][r + k][c];
        t1 += g * hq[1][r + k][c];
        t2 += g * hq[2][r + k][c];
      }
      const size_t idx = (size_t)gy * W + gx;
      const float m = M ? M[idx] : 1.f;
      const float xv = pred[base + idx] * m, yv = target[base + idx] * m;
      const float d = xv - yv;
      const float sgn = (float)((d > 0.f) - (d < 0.f));
      grad[base + idx] = m * (t0 + 2.f * xv * t1 + yv * t2 + 2.f * ca * d + cb * sgn);
    }
  }
}

int check_shape(const char* fn, int B, int C, int H, int W) {
  S3_REQUIRE(B > 0 && B <= 65535 / 3, "%s: B = %d, expected 1 .. %d", fn, B, 65535 / 3);
  S3_REQUIRE(C == 1 || C == 3, "%s: C = %d, expected 1 or 3", fn, C);
  S3_REQUIRE(H >= kTaps && W >= kTaps && H <= kMaxDim && W <= kMaxDim,
             "%s: image size %d x %d, expected %d .. %d per side", fn, H, W, kTaps, kMaxDim);
  return S3_OK;
}

Geo make_geo(int C, int H, int W) {
  Geo g;
  g.C = C;
  g.H = H;
  g.W = W;
  g.tiles_x = (int)s3::cdiv(W, kTW);
  g.tiles_y = (int)s3::cdiv(H, kTH);
  return g;
}

}  // namespace

extern "C" {

size_t s3p_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * C * s3::cdiv(W, kTW) * s3::cdiv(H, kTH) * S3P_NSUMS * sizeof(double);
}

size_t s3p_derivs_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)3 * B * C * H * W * sizeof(float);
}

void s3p_window(float* taps) {
  const Taps t = window();
  for (int k = 0; k < kTaps; ++k) taps[k] = t.g[k];
}

int s3p_forward(const float* pred, const float* target, const float* mask,
                int B, int C, int H, int W, int sample_covariance,
                float* smap, float* derivs, double* sums, void* workspace, void* stream) {
  if (int st = check_shape("s3p_forward", B, C, H, W)) return st;
  S3_REQUIRE(pred && target && sums, "s3p_forward: pred, target and sums must not be NULL");
  if (!workspace) {
    s3::set_error("s3p_forward: needs a workspace of %zu bytes",
                  s3p_workspace_bytes(B, C, H, W));
    return S3_ERR_WORKSPACE;
  }
  const Geo g = make_geo(C, H, W);
  const size_t n = (size_t)B * C * H * W;
  const float cn = sample_covariance ? 121.f / 120.f : 1.f;
  hipStream_t st = s3::as_stream(stream);
  double* partials = static_cast<double*>(workspace);
  const dim3 grid((unsigned)g.tiles_x, (unsigned)g.tiles_y, (unsigned)(B * C));
  hipLaunchKernelGGL(k_photo_fwd, grid, dim3(kThreads), 0, st, pred, target, mask, g, window(),
                     cn, smap, derivs, derivs ? derivs + n : nullptr,
                     derivs ? derivs + 2 * n : nullptr, partials);
  S3_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_photo_sums, dim3((unsigned)B), dim3(kThreads), 0, st, partials,
                     C * g.tiles_x * g.tiles_y, sums);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

int s3p_backward(const float* pred, const float* target, const float* mask,
                 const float* derivs, const float* wmap, const float* coef,
                 int B, int C, int H, int W, float* grad, void* stream) {
  if (int st = check_shape("s3p_backward", B, C, H, W)) return st;
  S3_REQUIRE(pred && target && derivs && coef && grad,
             "s3p_backward: pred, target, derivs, coef and grad must not be NULL");
  const Geo g = make_geo(C, H, W);
  const size_t n = (size_t)B * C * H * W;
  const dim3 grid((unsigned)g.tiles_x, (unsigned)g.tiles_y, (unsigned)(B * C));
  hipLaunchKernelGGL(k_photo_bwd, grid, dim3(kThreads), 0, s3::as_stream(stream), pred, target,
                     mask, derivs, derivs + n, derivs + 2 * n, wmap, coef, g, window(), grad);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

}  // extern "C"
