// Device-side frame ingest (include/s3i.h): Pillow's fixed-point 8-bit
// resample (horizontal pass -> uint8 -> vertical pass), the centre crop and
// ImgNorm of a batch of raw uint8 frames.  Integer arithmetic only: the
// normalised floats come out of a 256-entry table.
//
// One launch: a workgroup owns a tile of tw x th output pixels of one image.
// It stages the source rows and columns the tile's two filter windows reach
// into LDS with dword loads, runs the horizontal pass from LDS into a uint8
// LDS tile, then the vertical pass from that tile, and writes the planar
// float image and the interleaved uint8 image.  When even the smallest tile
// does not fit 64 KiB of LDS (very strong downscales) the two passes are two
// launches with the uint8 intermediate in the caller's workspace.
#include "common.hpp"
#include "s3i.h"

#include <atomic>

namespace {

constexpr int kThreads = 256;
constexpr int kPrecisionBits = 22;                 // Pillow: 32 - 8 - 2
constexpr int kHalf = 1 << (kPrecisionBits - 1);
constexpr size_t kLdsBudget = 64 * 1024;
constexpr int kMaxDim = 1 << 16;

std::atomic<int> g_path{0};

struct Geo {
  int B, in_h, in_w;
  int h_ksize, v_ksize;              // 0: no pass on that axis
  int crop_x0, crop_y0, crop_w, crop_h;
  int tw, th, lg_tw;                 // tile (tw a power of two <= kThreads)
  int max_span, max_rows;            // bounds of a tile's source span (pixels, rows)
  int raw_pitch;                     // bytes of a staged source row (multiple of 4)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ uint8_t clip8(int acc) {
  return (uint8_t)clampi(acc >> kPrecisionBits, 0, 255);
}

// Source span [lo, hi) of the outputs [first, first + n) of one axis.  The
// window starts and ends grow with the output index, so the span is the first
// window's start to the last window's end; it is clamped to the image and to
// the staged size, so that a table that disagrees with the sizes can make
// the result wrong but no access out of range.
__device__ __forceinline__ void tile_span(const int32_t* bounds, int first, int n, int in_size,
                                          int max_len, int& lo, int& hi) {
  if (bounds) {
    const int last = first + n - 1;
    lo = bounds[2 * first];
    hi = bounds[2 * last] + bounds[2 * last + 1];
  } else {
    lo = first;
    hi = first + n;
  }
  lo = clampi(lo, 0, in_size);
  hi = clampi(hi, lo, min(in_size, lo + max_len));
}

__global__ void __launch_bounds__(kThreads)
k_ingest(const uint8_t* __restrict__ src, const Geo g, const int32_t* __restrict__ hk,
         const int32_t* __restrict__ hb, const int32_t* __restrict__ vk,
         const int32_t* __restrict__ vb, const float* __restrict__ lut,
         float* __restrict__ img, uint8_t* __restrict__ uimg) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* s_lut = reinterpret_cast<float*>(smem);
  int32_t* s_hk = reinterpret_cast<int32_t*>(smem + 256 * sizeof(float));
  int32_t* s_vk = s_hk + g.tw * g.h_ksize;
  uint8_t* s_raw = reinterpret_cast<uint8_t*>(s_vk + g.th * g.v_ksize);
  const int mid_pitch = g.tw * 3;
  uint8_t* s_mid = s_raw + (size_t)g.max_rows * g.raw_pitch;

  const int tid = threadIdx.x, b = blockIdx.z;
  const int ox0 = blockIdx.x * g.tw, oy0 = blockIdx.y * g.th;
  const int tw = min(g.tw, g.crop_w - ox0), th = min(g.th, g.crop_h - oy0);
  const int X0 = g.crop_x0 + ox0, Y0 = g.crop_y0 + oy0;
  int xs_lo, xs_hi, ys_lo, ys_hi;
  tile_span(g.h_ksize ? hb : nullptr, X0, tw, g.in_w, g.max_span, xs_lo, xs_hi);
  tile_span(g.v_ksize ? vb : nullptr, Y0, th, g.in_h, g.max_rows, ys_lo, ys_hi);
  const int nrows = ys_hi - ys_lo;
  const int span_bytes = (xs_hi - xs_lo) * 3;

  for (int i = tid; i < 256; i += kThreads) s_lut[i] = lut[i];
  for (int i = tid; i < tw * g.h_ksize; i += kThreads) s_hk[i] = hk[(int64_t)X0 * g.h_ksize + i];
  for (int i = tid; i < th * g.v_ksize; i += kThreads) s_vk[i] = vk[(int64_t)Y0 * g.v_ksize + i];

  // Stage the span: one wave per source row, whole dwords.  A row starts at
  // any byte, so each staged row keeps its own misalignment `mis` in front.
  const uintptr_t base = reinterpret_cast<uintptr_t>(src);
  const uintptr_t end = base + (size_t)g.B * g.in_h * g.in_w * 3;
  const uintptr_t first = base + (((size_t)b * g.in_h + ys_lo) * g.in_w + xs_lo) * 3;
  const size_t row_bytes = (size_t)g.in_w * 3;
  for (int r = tid >> 6; r < nrows; r += kThreads >> 6) {
    const uintptr_t a0 = first + r * row_bytes;
    const int mis = (int)(a0 & 3);
    const int ndw = (mis + span_bytes + 3) >> 2;           // <= raw_pitch / 4
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_raw + (size_t)r * g.raw_pitch);
    for (int d = tid & 63; d < ndw; d += 64) {
      const uintptr_t a = a0 - mis + 4 * (uintptr_t)d;
      uint32_t v = 0;
      if (a >= base && a + 4 <= end) {
        v = *reinterpret_cast<const uint32_t*>(a);
      } else {   // the dword straddles the buffer's first or last byte
        for (int j = 0; j < 4; ++j)
          if (a + j >= base && a + j < end)
            v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(a + j)) << (8 * j);
      }
      dst[d] = v;
    }
  }
  __syncthreads();

  const int x = tid & (g.tw - 1);
  const int rstep = kThreads >> g.lg_tw;
  if (x < tw) {
    const int X = X0 + x;
    int xmin = X, cnt = 0;
    if (g.h_ksize) {
      xmin = clampi(hb[2 * X], xs_lo, xs_hi);
      cnt = clampi(hb[2 * X + 1], 0, min(g.h_ksize, xs_hi - xmin));
    }
    const int32_t* k = s_hk + x * g.h_ksize;
    for (int r = tid >> g.lg_tw; r < nrows; r += rstep) {
      const int mis = (int)((first + r * row_bytes) & 3);
      const uint8_t* p = s_raw + (size_t)r * g.raw_pitch + mis + (xmin - xs_lo) * 3;
      uint8_t* m = s_mid + r * mid_pitch + x * 3;
      if (g.h_ksize) {
        int a0 = kHalf, a1 = kHalf, a2 = kHalf;
        for (int j = 0; j < cnt; ++j) {
          const int c = k[j];
          a0 += (int)p[3 * j + 0] * c;
          a1 += (int)p[3 * j + 1] * c;
          a2 += (int)p[3 * j + 2] * c;
        }
        m[0] = clip8(a0);
        m[1] = clip8(a1);
        m[2] = clip8(a2);
      } else {
        m[0] = p[0];
        m[1] = p[1];
        m[2] = p[2];
      }
    }
  }
  __syncthreads();

  if (x < tw) {
    const int64_t plane = (int64_t)g.crop_h * g.crop_w;
    for (int y = tid >> g.lg_tw; y < th; y += rstep) {
      const int Y = Y0 + y;
      uint8_t o0, o1, o2;
      if (g.v_ksize) {
        const int ymin = clampi(vb[2 * Y], ys_lo, ys_hi);
        const int cnt = clampi(vb[2 * Y + 1], 0, min(g.v_ksize, ys_hi - ymin));
        const int32_t* k = s_vk + y * g.v_ksize;
        const uint8_t* p = s_mid + (ymin - ys_lo) * mid_pitch + x * 3;
        int a0 = kHalf, a1 = kHalf, a2 = kHalf;
        for (int j = 0; j < cnt; ++j) {
          const int c = k[j];
          a0 += (int)p[j * mid_pitch + 0] * c;
          a1 += (int)p[j * mid_pitch + 1] * c;
          a2 += (int)p[j * mid_pitch + 2] * c;
        }
        o0 = clip8(a0);
        o1 = clip8(a1);
        o2 = clip8(a2);
      } else {
        const uint8_t* p = s_mid + y * mid_pitch + x * 3;     // ys_lo == Y0
        o0 = p[0];
        o1 = p[1];
        o2 = p[2];
      }
      const int64_t pix = (int64_t)(oy0 + y) * g.crop_w + ox0 + x;
      float* o = img + (int64_t)b * 3 * plane + pix;
      o[0] = s_lut[o0];
      o[plane] = s_lut[o1];
      o[2 * plane] = s_lut[o2];
      if (uimg) {
        uint8_t* u = uimg + ((int64_t)b * plane + pix) * 3;
        u[0] = o0;
        u[1] = o1;
        u[2] = o2;
      }
    }
  }
}

// ---- two-launch path: the uint8 intermediate [B, in_h, crop_w, 3] in global
// memory (only the rows the vertical windows of the crop reach are written
// and read).
__global__ void __launch_bounds__(kThreads)
k_hpass(const uint8_t* __restrict__ src, const Geo g, const int32_t* __restrict__ hk,
        const int32_t* __restrict__ hb, const int32_t* __restrict__ vb,
        uint8_t* __restrict__ mid) {
  const int x = blockIdx.x * kThreads + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  if (x >= g.crop_w) return;
  int lo, hi;
  tile_span(g.v_ksize ? vb : nullptr, g.crop_y0, g.crop_h, g.in_h, g.in_h, lo, hi);
  if (r < lo || r >= hi) return;
  const int X = g.crop_x0 + x;
  const int xmin = clampi(hb[2 * X], 0, g.in_w);
  const int cnt = clampi(hb[2 * X + 1], 0, min(g.h_ksize, g.in_w - xmin));
  const uint8_t* p = src + (((int64_t)b * g.in_h + r) * g.in_w + xmin) * 3;
  const int32_t* k = hk + (int64_t)X * g.h_ksize;
  int a0 = kHalf, a1 = kHalf, a2 = kHalf;
  for (int j = 0; j < cnt; ++j) {
    const int c = k[j];
    a0 += (int)p[3 * j + 0] * c;
    a1 += (int)p[3 * j + 1] * c;
    a2 += (int)p[3 * j + 2] * c;
  }
  uint8_t* m = mid + (((int64_t)b * g.in_h + r) * g.crop_w + x) * 3;
  m[0] = clip8(a0);
  m[1] = clip8(a1);
  m[2] = clip8(a2);
}

// in: rows of `pitch` pixels, the crop's first column at pixel `xoff` (the
// intermediate: pitch = crop_w, xoff = 0; the source when there is no
// horizontal pass: pitch = in_w, xoff = crop_x0).
__global__ void __launch_bounds__(kThreads)
k_vpass(const uint8_t* __restrict__ in, int pitch, int xoff, const Geo g,
        const int32_t* __restrict__ vk, const int32_t* __restrict__ vb,
        const float* __restrict__ lut, float* __restrict__ img, uint8_t* __restrict__ uimg) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= g.crop_w) return;
  const int Y = g.crop_y0 + y;
  const int64_t stride = (int64_t)pitch * 3;
  uint8_t o0, o1, o2;
  if (g.v_ksize) {
    const int ymin = clampi(vb[2 * Y], 0, g.in_h);
    const int cnt = clampi(vb[2 * Y + 1], 0, min(g.v_ksize, g.in_h - ymin));
    const uint8_t* p = in + (((int64_t)b * g.in_h + ymin) * pitch + xoff + x) * 3;
    const int32_t* k = vk + (int64_t)Y * g.v_ksize;
    int a0 = kHalf, a1 = kHalf, a2 = kHalf;
    for (int j = 0; j < cnt; ++j) {
      const int c = k[j];
      a0 += (int)p[j * stride + 0] * c;
      a1 += (int)p[j * stride + 1] * c;
      a2 += (int)p[j * stride + 2] * c;
    }
    o0 = clip8(a0);
    o1 = clip8(a1);
    o2 = clip8(a2);
  } else {
    const uint8_t* p = in + (((int64_t)b * g.in_h + Y) * pitch + xoff + x) * 3;
    o0 = p[0];
    o1 = p[1];
    o2 = p[2];
  }
  const int64_t plane = (int64_t)g.crop_h * g.crop_w;
  const int64_t pix = (int64_t)y * g.crop_w + x;
  float* o = img + (int64_t)b * 3 * plane + pix;
  o[0] = lut[o0];
  o[plane] = lut[o1];
  o[2 * plane] = lut[o2];
  if (uimg) {
    uint8_t* u = uimg + ((int64_t)b * plane + pix) * 3;
    u[0] = o0;
    u[1] = o1;
    u[2] = o2;
  }
}

// Upper bound of the source span of n consecutive outputs of an axis
// resampled in_size -> out_size with ksize taps: the windows' centres are
// (n - 1) * in / out apart and a window is at most ksize wide (ksize =
// 2 ceil(support) + 1 >= 2 support + 1).  Without a pass the span is n.
int span_bound(int n, int in_size, int out_size, int ksize) {
  if (ksize == 0) return n;
  const int64_t s = ((int64_t)(n - 1) * in_size + out_size - 1) / out_size + ksize + 1;
  return (int)(s < in_size ? s : in_size);
}

// Tile shapes tried in turn; the first whose LDS need fits is used.
constexpr int kTiles[][2] = {{64, 16}, {64, 8}, {32, 8}, {32, 4}, {16, 4}, {16, 2}, {16, 1}};

size_t tile_lds(Geo& g, int tw, int th, int res_w, int res_h) {
  g.tw = tw;
  g.th = th;
  g.lg_tw = tw == 64 ? 6 : tw == 32 ? 5 : 4;
  g.max_span = span_bound(tw, g.in_w, res_w, g.h_ksize);
  g.max_rows = span_bound(th, g.in_h, res_h, g.v_ksize);
  g.raw_pitch = ((g.max_span * 3 + 3 + 3) / 4) * 4;
  return 256 * sizeof(float) + sizeof(int32_t) * ((size_t)tw * g.h_ksize + (size_t)th * g.v_ksize) +
         (size_t)g.max_rows * g.raw_pitch + (((size_t)g.max_rows * tw * 3 + 3) / 4) * 4;
}

// Picks the tile of the one-launch path into g; false if none fits.
bool pick_tile(Geo& g, int res_w, int res_h, size_t* lds) {
  for (const auto& t : kTiles) {
    const size_t need = tile_lds(g, t[0], t[1], res_w, res_h);
    if (need <= kLdsBudget) {
      *lds = need;
      return true;
    }
  }
  return false;
}

}  // namespace

extern "C" {

size_t s3i_workspace_bytes(int B, int in_h, int res_w) {
  if (B <= 0 || in_h <= 0 || res_w <= 0) return 0;
  return (size_t)B * in_h * res_w * 3;
}

int s3i_fused_fits(int in_h, int in_w, int h_ksize, int res_w, int v_ksize, int res_h) {
  if (in_h <= 0 || in_w <= 0 || res_w <= 0 || res_h <= 0 || h_ksize < 0 || v_ksize < 0) return 0;
  Geo g{};
  g.in_h = in_h;
  g.in_w = in_w;
  g.h_ksize = h_ksize;
  g.v_ksize = v_ksize;
  size_t lds;
  return pick_tile(g, res_w, res_h, &lds) ? 1 : 0;
}

void s3i_set_path(int path) { g_path.store(path); }

int s3i_ingest(const uint8_t* src, int B, int in_h, int in_w,
               const int32_t* hk, const int32_t* hb, int h_ksize, int res_w,
               const int32_t* vk, const int32_t* vb, int v_ksize, int res_h,
               int crop_x0, int crop_y0, int crop_w, int crop_h,
               const float* norm_lut, float* img, uint8_t* uimg,
               void* workspace, void* stream) {
  S3_REQUIRE(B > 0 && B <= 65535, "s3i_ingest: B = %d, expected 1 .. 65535", B);
  S3_REQUIRE(in_h > 0 && in_w > 0 && in_h <= kMaxDim && in_w <= kMaxDim,
             "s3i_ingest: input size %d x %d, expected 1 .. %d", in_h, in_w, kMaxDim);
  S3_REQUIRE(res_h > 0 && res_w > 0 && res_h <= kMaxDim && res_w <= kMaxDim,
             "s3i_ingest: resized size %d x %d, expected 1 .. %d", res_h, res_w, kMaxDim);
  S3_REQUIRE(crop_w > 0 && crop_h > 0, "s3i_ingest: crop size %d x %d is not positive",
             crop_h, crop_w);
  S3_REQUIRE(crop_x0 >= 0 && crop_y0 >= 0 && crop_x0 <= res_w - crop_w &&
                 crop_y0 <= res_h - crop_h,
             "s3i_ingest: crop [%d, %d) x [%d, %d) outside the resized image %d x %d", crop_y0,
             crop_y0 + crop_h, crop_x0, crop_x0 + crop_w, res_h, res_w);
  S3_REQUIRE(hk ? (hb && h_ksize > 0 && h_ksize <= kMaxDim) : res_w == in_w,
             "s3i_ingest: horizontal pass: %s", hk ? "bounds missing or ksize out of range"
                                                   : "no table, but res_w != in_w");
  S3_REQUIRE(vk ? (vb && v_ksize > 0 && v_ksize <= kMaxDim) : res_h == in_h,
             "s3i_ingest: vertical pass: %s", vk ? "bounds missing or ksize out of range"
                                                 : "no table, but res_h != in_h");
  S3_REQUIRE(src && norm_lut && img, "s3i_ingest: src, norm_lut and img must not be NULL");

  Geo g{};
  g.B = B;
  g.in_h = in_h;
  g.in_w = in_w;
  g.h_ksize = hk ? h_ksize : 0;
  g.v_ksize = vk ? v_ksize : 0;
  g.crop_x0 = crop_x0;
  g.crop_y0 = crop_y0;
  g.crop_w = crop_w;
  g.crop_h = crop_h;
  hipStream_t st = s3::as_stream(stream);

  size_t lds = 0;
  if (g_path.load() != 1 && pick_tile(g, res_w, res_h, &lds)) {
    const dim3 grid((unsigned)s3::cdiv(crop_w, g.tw), (unsigned)s3::cdiv(crop_h, g.th),
                    (unsigned)B);
    S3_REQUIRE(grid.y <= 65535, "s3i_ingest: crop_h = %d needs more than 65535 row tiles", crop_h);
    hipLaunchKernelGGL(k_ingest, grid, dim3(kThreads), lds, st, src, g, hk, hb, vk, vb, norm_lut,
                       img, uimg);
    S3_LAUNCH_CHECK();
    return S3_OK;
  }

  S3_REQUIRE(in_h <= 65535 && crop_h <= 65535,
             "s3i_ingest: two-launch path: %d source rows / %d output rows, at most 65535",
             in_h, crop_h);
  const unsigned gx = (unsigned)s3::cdiv(crop_w, kThreads);
  const uint8_t* vin = src;
  int pitch = in_w, xoff = crop_x0;
  if (hk) {
    if (!workspace) {
      s3::set_error("s3i_ingest: the two-launch path needs a workspace of %zu bytes",
                    s3i_workspace_bytes(B, in_h, res_w));
      return S3_ERR_WORKSPACE;
    }
    uint8_t* mid = static_cast<uint8_t*>(workspace);
    hipLaunchKernelGGL(k_hpass, dim3(gx, (unsigned)in_h, (unsigned)B), dim3(kThreads), 0, st, src,
                       g, hk, hb, vb, mid);
    S3_LAUNCH_CHECK();
    vin = mid;
    pitch = crop_w;
    xoff = 0;
  }
  hipLaunchKernelGGL(k_vpass, dim3(gx, (unsigned)crop_h, (unsigned)B), dim3(kThreads), 0, st, vin,
                     pitch, xoff, g, vk, vb, norm_lut, img, uimg);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

}  // extern "C"
