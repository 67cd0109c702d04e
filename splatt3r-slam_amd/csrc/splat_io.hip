// Gaussian map <-> 3DGS splat rows (include/s3w.h s3w_map_to_splats /
// s3w_map_from_splats); the per-Gaussian arithmetic is splat_math.hpp.
//
// k_map_to_splats    one Gaussian per thread: its 10 floats in, its 17-float
//                    row out.  A row is 68 bytes, so a wave writing its own
//                    rows would issue 17 dword stores of 68-byte stride; the
//                    workgroup's 256 rows are instead laid into LDS
//                    (row stride 17 dwords, odd: conflict-free) and written
//                    as the one contiguous 17,408-byte run they form, 16 bytes
//                    per lane (a workgroup's run starts at a multiple of
//                    17,408 bytes, so it is 16-byte aligned).
// k_map_from_splats  one Gaussian per thread: 14 floats in, the map's five
//                    fields out; thread 0 sets the count.
#include "common.hpp"
#include "s3w.h"
#include "splat_math.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kRow = s3w::kRowFloats;
constexpr int kRow14 = s3w::kRow14Floats;
static_assert((kThreads * kRow) % 4 == 0, "a workgroup's rows are whole float4s");

__global__ void __launch_bounds__(kThreads)
k_map_to_splats(const float* __restrict__ means, const float* __restrict__ cov,
                const float* __restrict__ colors, const float* __restrict__ opacities,
                const int64_t* __restrict__ n_dev, int64_t n_max, float scale_min,
                float* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) float tile[kThreads * kRow];
  int64_t n = n_max;
  if (n_dev) n = min(n, max(*n_dev, (int64_t)0));
  const int64_t base = (int64_t)blockIdx.x * kThreads;
  if (base >= n) return;  // workgroup-uniform
  const int live = (int)min((int64_t)kThreads, n - base);
  const int t = threadIdx.x;
  if (t < live) {
    const int64_t i = base + t;
    const float mean[3] = {means[i * 3 + 0], means[i * 3 + 1], means[i * 3 + 2]};
    const float c6[6] = {cov[i * 6 + 0], cov[i * 6 + 1], cov[i * 6 + 2],
                         cov[i * 6 + 3], cov[i * 6 + 4], cov[i * 6 + 5]};
    const float col[3] = {colors[i * 3 + 0], colors[i * 3 + 1], colors[i * 3 + 2]};
    float row[kRow];
    s3w::splat_row(mean, c6, col, opacities[i], scale_min, row);
#pragma unroll
    for (int k = 0; k < kRow; ++k) tile[t * kRow + k] = row[k];
  }
  __syncthreads();
  // the live rows are floats [0, live * 17) of the tile and of the
  // workgroup's run in `rows`: whole float4s, then at most 3 single floats
  const int nfloat = live * kRow;
  const int nvec = nfloat >> 2;
  float* __restrict__ out = rows + base * kRow;
  float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
  const float4* tile4 = reinterpret_cast<const float4*>(tile);
  for (int j = t; j < nvec; j += kThreads) out4[j] = tile4[j];
  const int tail = (nvec << 2) + t;
  if (tail < nfloat) out[tail] = tile[tail];
}

__global__ void __launch_bounds__(kThreads)
k_map_from_splats(s3w_map m, const float* __restrict__ rows14, int64_t n, int32_t kf) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) *m.n = n;
  if (i >= n) return;
  float r[kRow14];
#pragma unroll
  for (int k = 0; k < kRow14; ++k) r[k] = rows14[i * kRow14 + k];
  float mean[3], c6[6], col[3], op;
  s3w::splat_unpack(r, mean, c6, col, op);
#pragma unroll
  for (int k = 0; k < 3; ++k) m.means[i * 3 + k] = mean[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) m.cov_triu[i * 6 + k] = c6[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) m.colors[i * 3 + k] = col[k];
  m.opacities[i] = op;
  m.kf_id[i] = kf;
}

}  // namespace

extern "C" int s3w_map_to_splats(const float* means, const float* cov_triu, const float* colors,
                                 const float* opacities, const int64_t* n_dev, int64_t n_max,
                                 float scale_min, float* rows, void* stream) {
  s3::clear_error();
  S3_REQUIRE(n_max >= 0, "s3w_map_to_splats: n_max < 0");
  S3_REQUIRE(n_max < ((int64_t)1 << 31) * kThreads, "s3w_map_to_splats: n_max too large");
  S3_REQUIRE(scale_min > 0.0f, "s3w_map_to_splats: scale_min must be > 0");
  if (n_max == 0) return S3_OK;
  S3_REQUIRE(means && cov_triu && colors && opacities && rows,
             "s3w_map_to_splats: null argument");
  S3_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0,
             "s3w_map_to_splats: rows must be 16-byte aligned");
  k_map_to_splats<<<(unsigned)s3::cdiv(n_max, kThreads), kThreads, 0, s3::as_stream(stream)>>>(
      means, cov_triu, colors, opacities, n_dev, n_max, scale_min, rows);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" int s3w_map_from_splats(const s3w_map* map, const float* rows14, int64_t n,
                                   int32_t kf_idx, void* stream) {
  s3::clear_error();
  S3_REQUIRE(map && map->means && map->cov_triu && map->colors && map->opacities && map->kf_id &&
                 map->n && map->cap > 0,
             "s3w_map_from_splats: bad map");
  S3_REQUIRE(n >= 0, "s3w_map_from_splats: n < 0");
  S3_REQUIRE(n <= map->cap, "s3w_map_from_splats: n = %lld exceeds the map's capacity %lld",
             (long long)n, (long long)map->cap);
  S3_REQUIRE(n == 0 || rows14, "s3w_map_from_splats: null rows");
  // n == 0 still launches one workgroup: it sets the count
  const int64_t blocks = n > 0 ? s3::cdiv(n, kThreads) : 1;
  k_map_from_splats<<<(unsigned)blocks, kThreads, 0, s3::as_stream(stream)>>>(*map, rows14, n,
                                                                             kf_idx);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
