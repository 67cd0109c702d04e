// Depth loss and depth-metric sums (include/s3z.h), written for gfx950.
//
// Forward:  k_depth_fwd, one 256-lane workgroup per 64 x 8 tile of one image.
//           Every pixel of the tile, of the column right of it and of the row
//           below it is evaluated once (depth_loss_math.hpp pixel()) and its
//           (w, r) goes to LDS; the tile's pixels add their per-pixel terms
//           and write rmap on the way.  After the barrier every tile pixel
//           adds its right and its lower pair from LDS.  Each workgroup writes
//           its S3Z_NSUMS partial sums (double; lanes by an xor butterfly,
//           then the four waves in order); k_depth_sums adds an image's
//           partials in double in a fixed order.  No floating-point atomics.
// Backward: k_depth_bwd, same tiling with a one-pixel halo on all four sides:
//           (w, r) of tile + halo to LDS, then every tile pixel gathers its
//           four neighbours (no scatter) and writes dL/dD and dL/dA.
// The arithmetic is double for reproducibility against the float64 reference;
// the pass moves 16 B in and at most 12 B out per pixel (see DESIGN 6u for
// which of the two bounds it).
#include <cmath>

#include "arg_check.hpp"
#include "common.hpp"
#include "depth_loss_math.hpp"
#include "s3z.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTW = S3Z_TILE_W;
constexpr int kTH = S3Z_TILE_H;
constexpr int kRows = kTH / (kThreads / kTW);   // tile rows per lane
constexpr int kMaxDim = 1 << 15;
constexpr int kMaxBatch = 65535;

static_assert(kTW == 64 && kThreads % kTW == 0 && kTH % (kThreads / kTW) == 0,
              "tile / workgroup shape");

struct Geo {
  int H, W;
  int tiles_x, tiles_y;
};

__global__ __launch_bounds__(kThreads) void k_depth_fwd(
    const float* __restrict__ depth, const float* __restrict__ alpha,
    const float* __restrict__ target, const float* __restrict__ weight,
    const float* __restrict__ scale, Geo geo, double alpha_min, float* __restrict__ rmap,
    double* __restrict__ partials) {
  __shared__ double sw[kTH + 1][kTW + 1];
  __shared__ double sr[kTH + 1][kTW + 1];
  __shared__ double red[kThreads / 64][S3Z_NSUMS];

  const int tid = threadIdx.x;
  const int H = geo.H, W = geo.W;
  const int b = blockIdx.z;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const size_t base = (size_t)b * H * W;
  const double s = scale ? (double)scale[b] : 1.0;

  double acc[S3Z_NSUMS];
#pragma unroll
  for (int k = 0; k < S3Z_NSUMS; ++k) acc[k] = 0.0;

  // tile, the column right of it and the row below it
  for (int i = tid; i < (kTH + 1) * (kTW + 1); i += kThreads) {
    const int r = i / (kTW + 1), c = i - r * (kTW + 1);
    const int gy = y0 + r, gx = x0 + c;
    s3z::Pixel px{0.0, 0.0, 0.0, 0.0};
    if (gy < H && gx < W) {
      const size_t idx = base + (size_t)gy * W + gx;
      const float z = target[idx];
      px = s3z::pixel(depth[idx], alpha[idx], z, weight ? weight[idx] : 1.f, s, alpha_min);
      if (r < kTH && c < kTW) {
        if (rmap) rmap[idx] = (float)px.r;
        if (px.w > 0.0) {
          double t[S3Z_NSUMS];
          s3z::terms(px, z, t);
#pragma unroll
          for (int k = 0; k < S3Z_NSUMS; ++k) acc[k] += t[k];
        }
      }
    }
    sw[r][c] = px.w;
    sr[r][c] = px.r;
  }
  __syncthreads();

  // the pairs a tile pixel owns: with its right, then with its lower neighbour
  const int c = tid & (kTW - 1);
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int r = (tid / kTW) + j * (kThreads / kTW);
    const double w = sw[r][c], rp = sr[r][c];
    if (w > 0.0) {
      const double wr = sw[r][c + 1], wd = sw[r + 1][c];
      if (wr > 0.0) {
        acc[S3Z_SUM_GRAD] += s3z::pair_term(w, rp, wr, sr[r][c + 1]);
        acc[S3Z_SUM_WG] += s3z::pair_weight(w, wr);
      }
      if (wd > 0.0) {
        acc[S3Z_SUM_GRAD] += s3z::pair_term(w, rp, wd, sr[r + 1][c]);
        acc[S3Z_SUM_WG] += s3z::pair_weight(w, wd);
      }
    }
  }

  // lanes (xor butterfly), then the four waves in order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < S3Z_NSUMS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (tid < S3Z_NSUMS) {
    double v = red[0][tid];
    for (int w = 1; w < kThreads / 64; ++w) v += red[w][tid];
    const size_t tile = (size_t)blockIdx.y * geo.tiles_x + blockIdx.x;
    partials[((size_t)b * geo.tiles_x * geo.tiles_y + tile) * S3Z_NSUMS + tid] = v;
  }
}

// One workgroup per batch image: lane t adds partials t, t + 256, ... in
// order, then a fixed LDS tree.
__global__ __launch_bounds__(kThreads) void k_depth_sums(const double* __restrict__ partials,
                                                         int n, double* __restrict__ sums) {
  __shared__ double red[kThreads][S3Z_NSUMS];
  const int tid = threadIdx.x;
  const double* p = partials + (size_t)blockIdx.x * n * S3Z_NSUMS;
  double acc[S3Z_NSUMS];
#pragma unroll
  for (int k = 0; k < S3Z_NSUMS; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += kThreads)
#pragma unroll
    for (int k = 0; k < S3Z_NSUMS; ++k) acc[k] += p[(size_t)i * S3Z_NSUMS + k];
#pragma unroll
  for (int k = 0; k < S3Z_NSUMS; ++k) red[tid][k] = acc[k];
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int k = 0; k < S3Z_NSUMS; ++k) red[tid][k] += red[tid + o][k];
    __syncthreads();
  }
  if (tid < S3Z_NSUMS) sums[(size_t)blockIdx.x * S3Z_NSUMS + tid] = red[0][tid];
}

__global__ __launch_bounds__(kThreads) void k_depth_bwd(
    const float* __restrict__ depth, const float* __restrict__ alpha,
    const float* __restrict__ target, const float* __restrict__ weight,
    const float* __restrict__ scale, const float* __restrict__ coef, Geo geo, double alpha_min,
    float* __restrict__ grad_depth, float* __restrict__ grad_alpha) {
  __shared__ double sw[kTH + 2][kTW + 2];
  __shared__ double sr[kTH + 2][kTW + 2];

  const int tid = threadIdx.x;
  const int H = geo.H, W = geo.W;
  const int b = blockIdx.z;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const size_t base = (size_t)b * H * W;
  const double s = scale ? (double)scale[b] : 1.0;
  const double c_abs = (double)coef[b * 3 + 0], c_sq = (double)coef[b * 3 + 1],
               c_grad = (double)coef[b * 3 + 2];

  // tile plus one pixel on every side
  for (int i = tid; i < (kTH + 2) * (kTW + 2); i += kThreads) {
    const int r = i / (kTW + 2), c = i - r * (kTW + 2);
    const int gy = y0 + r - 1, gx = x0 + c - 1;
    s3z::Pixel px{0.0, 0.0, 0.0, 0.0};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t idx = base + (size_t)gy * W + gx;
      px = s3z::pixel(depth[idx], alpha[idx], target[idx], weight ? weight[idx] : 1.f, s,
                      alpha_min);
    }
    sw[r][c] = px.w;
    sr[r][c] = px.r;
  }
  __syncthreads();

  const int c = tid & (kTW - 1);
  const int gx = x0 + c;
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int r = (tid / kTW) + j * (kThreads / kTW);
    const int gy = y0 + r;
    if (gy < H && gx < W) {
      const size_t idx = base + (size_t)gy * W + gx;
      const int lr = r + 1, lc = c + 1;
      const double w = sw[lr][lc];
      float gd = 0.f, ga = 0.f;
      if (w > 0.0) {
        const double d = s3z::dl_dr(w, sr[lr][lc], sw[lr][lc - 1], sr[lr][lc - 1], sw[lr][lc + 1],
                                    sr[lr][lc + 1], sw[lr - 1][lc], sr[lr - 1][lc], sw[lr + 1][lc],
                                    sr[lr + 1][lc], c_abs, c_sq, c_grad);
        s3z::grads(d, depth[idx], alpha[idx], s, gd, ga);
      }
      grad_depth[idx] = gd;
      grad_alpha[idx] = ga;
    }
  }
}

int check_common(const char* fn, const float* depth, const float* alpha, const float* target,
                 const float* weight, const float* scale, int B, int H, int W, double alpha_min) {
  S3_REQUIRE(B > 0 && B <= kMaxBatch, "%s: B = %d, expected 1 .. %d", fn, B, kMaxBatch);
  S3_REQUIRE(H >= 1 && W >= 1 && H <= kMaxDim && W <= kMaxDim,
             "%s: image size %d x %d, expected 1 .. %d per side", fn, H, W, kMaxDim);
  S3_REQUIRE(alpha_min >= 0.0 && alpha_min <= 1.7976931348623157e308,
             "%s: alpha_min must be >= 0 and finite", fn);
  S3_REQUIRE(depth && alpha && target, "%s: depth, alpha and target must not be NULL", fn);
  S3_REQUIRE(s3::aligned(depth, 4) && s3::aligned(alpha, 4) && s3::aligned(target, 4) &&
                 s3::aligned(weight, 4) && s3::aligned(scale, 4),
             "%s: a float input is not 4-byte aligned", fn);
  return S3_OK;
}

// the output [out, out + bytes) is none of the inputs
int check_output(const char* fn, const char* name, const void* out, size_t bytes,
                 const float* depth, const float* alpha, const float* target,
                 const float* weight, const float* scale, int B) {
  S3_REQUIRE(s3::aligned(out, 4), "%s: %s is not 4-byte aligned", fn, name);
  const void* in[4] = {depth, alpha, target, weight};
  for (const void* p : in)
    S3_REQUIRE(!p || !s3::overlap(out, bytes, p, bytes), "%s: %s overlaps an input", fn, name);
  S3_REQUIRE(!scale || !s3::overlap(out, bytes, scale, (size_t)B * sizeof(float)),
             "%s: %s overlaps scale", fn, name);
  return S3_OK;
}

Geo make_geo(int H, int W) {
  Geo g;
  g.H = H;
  g.W = W;
  g.tiles_x = (int)s3::cdiv(W, kTW);
  g.tiles_y = (int)s3::cdiv(H, kTH);
  return g;
}

}  // namespace

extern "C" {

size_t s3z_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * s3::cdiv(W, kTW) * s3::cdiv(H, kTH) * S3Z_NSUMS * sizeof(double);
}

int s3z_forward(const float* depth, const float* alpha, const float* target,
                const float* weight, const float* scale, int B, int H, int W,
                double alpha_min, float* rmap, double* sums, void* workspace, void* stream) {
  const char* fn = "s3z_forward";
  if (int st = check_common(fn, depth, alpha, target, weight, scale, B, H, W, alpha_min)) return st;
  S3_REQUIRE(sums && s3::aligned(sums, 8), "%s: sums must not be NULL and 8-byte aligned", fn);
  const size_t bytes = (size_t)B * H * W * sizeof(float);
  if (rmap)
    if (int st = check_output(fn, "rmap", rmap, bytes, depth, alpha, target, weight, scale, B))
      return st;
  if (!workspace || !s3::aligned(workspace, 8)) {
    s3::set_error("%s: needs an 8-byte aligned workspace of %zu bytes", fn,
                  s3z_workspace_bytes(B, H, W));
    return S3_ERR_WORKSPACE;
  }
  const Geo g = make_geo(H, W);
  hipStream_t st = s3::as_stream(stream);
  double* partials = static_cast<double*>(workspace);
  const dim3 grid((unsigned)g.tiles_x, (unsigned)g.tiles_y, (unsigned)B);
  hipLaunchKernelGGL(k_depth_fwd, grid, dim3(kThreads), 0, st, depth, alpha, target, weight,
                     scale, g, alpha_min, rmap, partials);
  S3_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_depth_sums, dim3((unsigned)B), dim3(kThreads), 0, st, partials,
                     g.tiles_x * g.tiles_y, sums);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

int s3z_backward(const float* depth, const float* alpha, const float* target,
                 const float* weight, const float* scale, const float* coef,
                 int B, int H, int W, double alpha_min,
                 float* grad_depth, float* grad_alpha, void* stream) {
  const char* fn = "s3z_backward";
  if (int st = check_common(fn, depth, alpha, target, weight, scale, B, H, W, alpha_min)) return st;
  S3_REQUIRE(coef && grad_depth && grad_alpha,
             "%s: coef, grad_depth and grad_alpha must not be NULL", fn);
  S3_REQUIRE(s3::aligned(coef, 4), "%s: coef is not 4-byte aligned", fn);
  const size_t bytes = (size_t)B * H * W * sizeof(float);
  if (int st = check_output(fn, "grad_depth", grad_depth, bytes, depth, alpha, target, weight,
                            scale, B))
    return st;
  if (int st = check_output(fn, "grad_alpha", grad_alpha, bytes, depth, alpha, target, weight,
                            scale, B))
    return st;
  S3_REQUIRE(!s3::overlap(grad_depth, bytes, grad_alpha, bytes),
             "%s: grad_depth and grad_alpha overlap each other", fn);
  const Geo g = make_geo(H, W);
  const dim3 grid((unsigned)g.tiles_x, (unsigned)g.tiles_y, (unsigned)B);
  hipLaunchKernelGGL(k_depth_bwd, grid, dim3(kThreads), 0, s3::as_stream(stream), depth, alpha,
                     target, weight, scale, coef, g, alpha_min, grad_depth, grad_alpha);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

}  // extern "C"
