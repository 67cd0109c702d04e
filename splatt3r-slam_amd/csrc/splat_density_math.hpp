// Per-Gaussian arithmetic of adaptive density control (splat_density.hip,
// include/s3d.h), host + device so a host program can restate it
// (tests/native/splat_density_host.cpp).
//
// A parameter row is the 14-float rows14 layout of splat_opt_math.hpp:
//   x y z | f_dc_0..2 | logit opacity | log scale_0..2 | rot w x y z (raw).
//
// decide()      one decision per row: prune, keep, clone or split
// normals3()    three standard normals of (row, pass, child, seed):
//               Philox4x32-10, Box-Muller in double, rounded to float32 once
// split_child() child k of a split row
// Build with -ffp-contract=off: every product and sum rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "splat_opt_math.hpp"

#define S3D_HD __host__ __device__ __forceinline__

namespace s3d {

constexpr int kRow = s3o::kRow;
constexpr float kFltMax = 3.402823466e+38f;

// decision codes
constexpr int kPrune = 0, kKeep = 1, kClone = 2, kSplit = 3;

// float32(log 1.6): a split child's log scale is the parent's minus this
constexpr float kLogSplit = 0.4700036292457356f;

struct Params {
  float grad_threshold, split_scale, min_opacity, max_scale;
  int32_t max_screen_radius;
};

S3D_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
}

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2] -> c[4].
S3D_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// Three standard normals for child k of `row` in density pass `pass`:
// counter (row lo32, row hi32, pass, k), key (seed lo32, seed hi32); the words
// become u_j = (x_j + 0.5) / 2^32 in (0, 1); two Box-Muller pairs in double,
// (sqrt(-2 ln u0) cos 2 pi u1, ... sin 2 pi u1) and the same of (u2, u3); each
// rounded to float32 once; the first three are returned.
S3D_HD void normals3(int64_t row, uint32_t pass, uint32_t k, uint64_t seed, float (&e)[3]) {
  uint32_t c[4] = {(uint32_t)((uint64_t)row & 0xffffffffu), (uint32_t)((uint64_t)row >> 32), pass,
                   k};
  philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  constexpr double kInv = 1.0 / 4294967296.0, kTwoPi = 6.283185307179586476925286766559;
  const double u0 = ((double)c[0] + 0.5) * kInv, u1 = ((double)c[1] + 0.5) * kInv;
  const double u2 = ((double)c[2] + 0.5) * kInv, u3 = ((double)c[3] + 0.5) * kInv;
  const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
  e[0] = (float)(r0 * cos(kTwoPi * u1));
  e[1] = (float)(r0 * sin(kTwoPi * u1));
  e[2] = (float)(r1 * cos(kTwoPi * u3));
}

S3D_HD bool row_finite(const float (&r)[kRow]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kRow; ++k) ok = ok && fabsf(r[k]) <= kFltMax;
  return ok;
}

// The decision of one row, in this order: prune (a non-finite entry,
// o < min_opacity, smax > max_scale when max_scale > 0, max_radii >
// max_screen_radius when that is > 0); grow when avg >= grad_threshold, split
// if smax > split_scale, else clone; else keep.  o = sigmoid(logit) and
// s_k = exp(log scale_k) are splat_opt_math.hpp's activations (formed in
// double, rounded once, render_scale 1: world units); avg = grad_accum / denom
// in float32, 0 when denom <= 0.
S3D_HD int decide(const float (&r)[kRow], float grad_accum, int32_t denom, int32_t max_radii,
                  const Params& p) {
  if (!row_finite(r)) return kPrune;
  float mean[3], sh[3], o, sc[3], q[4];
  s3o::activate(r, 1.0f, mean, sh, o, sc, q);
  const float smax = fmaxf(sc[0], fmaxf(sc[1], sc[2]));
  if (o < p.min_opacity) return kPrune;
  if (p.max_scale > 0.0f && smax > p.max_scale) return kPrune;
  if (p.max_screen_radius > 0 && max_radii > p.max_screen_radius) return kPrune;
  const float avg = denom > 0 ? grad_accum / (float)denom : 0.0f;
  if (avg >= p.grad_threshold) return smax > p.split_scale ? kSplit : kClone;
  return kKeep;
}

// Child k of a split row: mean = mu + R (s * eps_k) in float32, R of q / |q|
// (a zero quaternion is the identity), log scale -= float32(log 1.6); f_dc,
// the logit and the raw quaternion are the parent's bits.
S3D_HD void split_child(const float (&r)[kRow], int64_t row, uint32_t pass, uint32_t k,
                        uint64_t seed, float (&c)[kRow]) {
  float mean[3], sh[3], o, sc[3], q[4], e[3];
  s3o::activate(r, 1.0f, mean, sh, o, sc, q);
  normals3(row, pass, k, seed, e);
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float R[3][3] = {
      {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - w * z), 2.0f * (x * z + w * y)},
      {2.0f * (x * y + w * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - w * x)},
      {2.0f * (x * z - w * y), 2.0f * (y * z + w * x), 1.0f - 2.0f * (x * x + y * y)}};
  const float d[3] = {sc[0] * e[0], sc[1] * e[1], sc[2] * e[2]};
#pragma unroll
  for (int j = 0; j < kRow; ++j) c[j] = r[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    c[j] = r[j] + ((R[j][0] * d[0] + R[j][1] * d[1]) + R[j][2] * d[2]);
    c[7 + j] = r[7 + j] - kLogSplit;
  }
}

// The gradient-norm statistic of one visible row: sqrt(dx^2 + dy^2), or a
// negative value when dx or dy is not finite (the row is then left alone).
S3D_HD float grad_norm2d(float dx, float dy) {
  if (!(fabsf(dx) <= kFltMax && fabsf(dy) <= kFltMax)) return -1.0f;
  return sqrtf(dx * dx + dy * dy);
}

}  // namespace s3d
