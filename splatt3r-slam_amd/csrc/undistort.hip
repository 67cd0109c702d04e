// Lens undistortion (include/s3u.h): cv2's 8-bit INTER_LINEAR remap with a
// constant-0 border, for a batch of frames that share one pair of maps.
//
// A thread owns four consecutive output pixels of the flattened
// [out_h * out_w] frame: it reads their map entries once (two float4 loads),
// quantises them to 1/32 pixel, and keeps the four tap weights and the two
// tap rows' addresses in registers.  It then walks the B frames: per pixel
// the two taps of a row are adjacent in memory (2 C bytes), so each row is
// one load of whole dwords from the dword boundary below it (3 dwords for
// C = 3, 2 for C = 1) and a funnel shift -- two loads a pixel, not 4 C byte
// loads; the source (about 1 MB per frame) is served by L2.  Then the integer
// blend, and the four pixels' 12 output bytes written as three dwords.  A
// tap outside the image gets weight 0 and its address is clamped into the
// image, so every load is in range whatever the map holds.  Integer
// arithmetic only after the one rint(v * 32).
#include "common.hpp"
#include "s3u.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                  // pixels per thread: 12 bytes = 3 dwords
constexpr int kInterBits = 5;            // cv2 INTER_BITS
constexpr int kInterTab = 1 << kInterBits;
constexpr int kMaxSrcDim = 32767;        // ix, iy live in the short range
constexpr int kMaxOutDim = 1 << 16;

struct Taps {
  int off0, off1;                        // pixel offsets of the two tap rows' left taps, in range
  int w00, w01, w10, w11;                // weights, sum 1024; 0 for a tap outside
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// cv2: sx = cvRound(v * INTER_TAB_SIZE) (nearest, ties to even); the product
// is exact in float32.  ix = saturate_cast<short>(sx >> INTER_BITS).
//
// The two taps of a row are read as one run of 2 C bytes that starts at the
// left tap's column clamped into the image.  At ix = -1 that column is the
// RIGHT tap's (column 0), so its weights move to the left slot; at ix = W - 1
// the right slot's weight is 0 and what the run holds there does not matter.
__device__ __forceinline__ Taps make_taps(float mx, float my, int H, int W) {
  const int sx = __float2int_rn(mx * (float)kInterTab);
  const int sy = __float2int_rn(my * (float)kInterTab);
  const int ix = clampi(sx >> kInterBits, -32768, 32767);
  const int iy = clampi(sy >> kInterBits, -32768, 32767);
  const int fx = sx & (kInterTab - 1), fy = sy & (kInterTab - 1);
  const bool x0 = ix >= 0 && ix < W, x1 = ix + 1 >= 0 && ix + 1 < W;
  const bool y0 = iy >= 0 && iy < H, y1 = iy + 1 >= 0 && iy + 1 < H;
  int wx0 = x0 ? kInterTab - fx : 0, wx1 = x1 ? fx : 0;
  if (ix < 0) {                          // ix == -1 is the only case with wx1 != 0
    wx0 = wx1;
    wx1 = 0;
  }
  const int wy0 = y0 ? kInterTab - fy : 0, wy1 = y1 ? fy : 0;
  const int cx = clampi(ix, 0, W - 1);
  Taps t;
  t.off0 = clampi(iy, 0, H - 1) * W + cx;
  t.off1 = clampi(iy + 1, 0, H - 1) * W + cx;
  t.w00 = wx0 * wy0;
  t.w01 = wx1 * wy0;
  t.w10 = wx0 * wy1;
  t.w11 = wx1 * wy1;
  return t;
}

__device__ __forceinline__ uint32_t blend(const Taps& t, uint32_t p00, uint32_t p01, uint32_t p10,
                                          uint32_t p11) {
  return (uint32_t)(t.w00 * (int)p00 + t.w01 * (int)p01 + t.w10 * (int)p10 + t.w11 * (int)p11 +
                    512) >> 10;
}

// The 8 bytes at src + off (any alignment) as two dwords, read as N whole
// dwords from the dword boundary below them (N = 2 serves the first 5 bytes,
// N = 3 all 8).  The source buffer is [src, src + total): a run whose dwords
// would leave it -- only at the buffer's first and last bytes -- is read
// bytewise, bytes outside as 0 (they only ever meet a weight of 0).
template <int N>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ src, int64_t off,
                                         int64_t total, uint32_t& lo, uint32_t& hi) {
  const int mis = (int)((reinterpret_cast<uintptr_t>(src) + (uintptr_t)off) & 3);
  const int64_t s = off - mis;           // >= -3
  uint32_t d[3] = {0u, 0u, 0u};
  if (s >= 0 && s + 4 * N <= total) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + s);
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] = p[j];
  } else {
    for (int j = 0; j < 4 * N; ++j)
      if (s + j >= 0 && s + j < total) d[j >> 2] |= (uint32_t)src[s + j] << (8 * (j & 3));
  }
  const int sh = 8 * mis;
  lo = (uint32_t)((((uint64_t)d[1] << 32) | d[0]) >> sh);
  hi = (uint32_t)((((uint64_t)d[2] << 32) | d[1]) >> sh);
}

// The three output bytes of one pixel of the frame at byte offset f of src.
template <int C>
__device__ __forceinline__ void pixel(const uint8_t* __restrict__ src, int64_t f, int64_t total,
                                      const Taps& t, uint32_t (&o)[3]) {
  uint32_t r0, r1, h0, h1;
  if (C == 1) {                          // 2 bytes a row
    load_run<2>(src, f + t.off0, total, r0, h0);
    load_run<2>(src, f + t.off1, total, r1, h1);
    o[0] = o[1] = o[2] = blend(t, r0 & 255u, (r0 >> 8) & 255u, r1 & 255u, (r1 >> 8) & 255u);
  } else {                               // 6 bytes a row: the left tap's RGB, the right tap's
    load_run<3>(src, f + (int64_t)t.off0 * 3, total, r0, h0);
    load_run<3>(src, f + (int64_t)t.off1 * 3, total, r1, h1);
    o[0] = blend(t, r0 & 255u, r0 >> 24, r1 & 255u, r1 >> 24);
    o[1] = blend(t, (r0 >> 8) & 255u, h0 & 255u, (r1 >> 8) & 255u, h1 & 255u);
    o[2] = blend(t, (r0 >> 16) & 255u, (h0 >> 8) & 255u, (r1 >> 16) & 255u, (h1 >> 8) & 255u);
  }
}

template <int C>
__global__ void __launch_bounds__(kThreads)
k_remap(const uint8_t* __restrict__ src, int B, int H, int W, const float* __restrict__ mapx,
        const float* __restrict__ mapy, int64_t npix, int maps_vec, uint8_t* __restrict__ dst) {
  const int64_t p0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kPix;
  if (p0 >= npix) return;
  const int n = (int)min((int64_t)kPix, npix - p0);

  float mx[kPix], my[kPix];
  if (n == kPix && maps_vec) {           // p0 is a multiple of 4: 16-byte aligned
    const float4 vx = *reinterpret_cast<const float4*>(mapx + p0);
    const float4 vy = *reinterpret_cast<const float4*>(mapy + p0);
    mx[0] = vx.x, mx[1] = vx.y, mx[2] = vx.z, mx[3] = vx.w;
    my[0] = vy.x, my[1] = vy.y, my[2] = vy.z, my[3] = vy.w;
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      mx[i] = i < n ? mapx[p0 + i] : 0.f;
      my[i] = i < n ? mapy[p0 + i] : 0.f;
    }
  }
  Taps t[kPix];
#pragma unroll
  for (int i = 0; i < kPix; ++i) t[i] = make_taps(mx[i], my[i], H, W);

  const int64_t src_frame = (int64_t)H * W * C, dst_frame = npix * 3;
  const int64_t total = B * src_frame;
  for (int b = 0; b < B; ++b) {
    uint32_t o[kPix][3];
#pragma unroll
    for (int i = 0; i < kPix; ++i) pixel<C>(src, b * src_frame, total, t[i], o[i]);
    uint8_t* out = dst + b * dst_frame + p0 * 3;
    if (n == kPix && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
      uint32_t* q = reinterpret_cast<uint32_t*>(out);
      q[0] = o[0][0] | o[0][1] << 8 | o[0][2] << 16 | o[1][0] << 24;
      q[1] = o[1][1] | o[1][2] << 8 | o[2][0] << 16 | o[2][1] << 24;
      q[2] = o[2][2] | o[3][0] << 8 | o[3][1] << 16 | o[3][2] << 24;
    } else {                             // the frame's tail, or an unaligned frame
      for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) out[i * 3 + k] = (uint8_t)o[i][k];
    }
  }
}

}  // namespace

extern "C" {

int s3u_remap(const uint8_t* src, int B, int H, int W, int C, const float* mapx,
              const float* mapy, int out_h, int out_w, uint8_t* dst, void* stream) {
  S3_REQUIRE(src && mapx && mapy && dst,
             "s3u_remap: null pointer (src, mapx, mapy and dst must not be NULL)");
  S3_REQUIRE(C == 1 || C == 3, "s3u_remap: C = %d, expected 1 or 3", C);
  S3_REQUIRE(B > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0,
             "s3u_remap: non-positive size (B = %d, source %d x %d, output %d x %d)", B, H, W,
             out_h, out_w);
  S3_REQUIRE(H <= kMaxSrcDim && W <= kMaxSrcDim,
             "s3u_remap: source size %d x %d, at most %d", H, W, kMaxSrcDim);
  S3_REQUIRE(out_h <= kMaxOutDim && out_w <= kMaxOutDim,
             "s3u_remap: output size %d x %d, at most %d", out_h, out_w, kMaxOutDim);
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  const uint64_t src_bytes = (uint64_t)B * H * W * C, dst_bytes = (uint64_t)B * out_h * out_w * 3;
  S3_REQUIRE(s0 + src_bytes <= d0 || d0 + dst_bytes <= s0, "s3u_remap: dst overlaps src");

  const int64_t npix = (int64_t)out_h * out_w;
  const int64_t blocks = s3::cdiv(s3::cdiv(npix, kPix), kThreads);
  const int maps_vec = ((reinterpret_cast<uintptr_t>(mapx) | reinterpret_cast<uintptr_t>(mapy)) & 15) == 0;
  hipStream_t st = s3::as_stream(stream);
  if (C == 1)
    hipLaunchKernelGGL(k_remap<1>, dim3((unsigned)blocks), dim3(kThreads), 0, st, src, B, H, W,
                       mapx, mapy, npix, maps_vec, dst);
  else
    hipLaunchKernelGGL(k_remap<3>, dim3((unsigned)blocks), dim3(kThreads), 0, st, src, B, H, W,
                       mapx, mapy, npix, maps_vec, dst);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

}  // extern "C"
