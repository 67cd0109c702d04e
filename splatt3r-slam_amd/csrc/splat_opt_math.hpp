// Per-Gaussian arithmetic of the splat optimiser (splat_opt.hip, include/s3o.h
// s3o_activate / s3o_adam_step), host + device so a host program can restate
// it (tests/native/splat_opt_host.cpp).
//
// A parameter row is the 14-float rows14 layout of s3w_map_from_splats:
//   x y z | f_dc_0..2 | logit opacity | log scale_0..2 | rot w x y z (raw).
// Five parameter groups, each with its own learning rate: means, f_dc,
// opacity, scale, rotation.
//
// Activation, with the scale-invariant render factor s (1 / near):
//   means3D = s xyz, shs = f_dc, opacity = sigmoid(logit),
//   scales = s exp(log scale), rotations = q / |q| (r, x, y, z), a zero
//   quaternion being the identity (as s3w::splat_unpack reads it).
// Chain rule from the rasterizer's five gradients to the row:
//   g_xyz = s dmeans3D, g_fdc = dsh, g_logit = dop o (1 - o),
//   g_logscale = dscales scales, g_q = (dr - qh (qh . dr)) / |q| (zero for a
//   zero quaternion).
// Adam is torch.optim.Adam without weight decay or amsgrad.
// Build with -ffp-contract=off: every product and sum rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "splat_math.hpp"

#define S3O_HD __host__ __device__ __forceinline__

namespace s3o {

constexpr int kRow = s3w::kRow14Floats;
constexpr int kGroups = 5;  // means, f_dc, opacity, scale, rotation

// Parameter group of row entry k (constant-folded where k is).
S3O_HD constexpr int group_of(int k) { return k < 3 ? 0 : k < 6 ? 1 : k < 7 ? 2 : k < 10 ? 3 : 4; }

// sigmoid(x) and its derivative o (1 - o), both from e = exp(-|x|): 1 - o is
// never formed by subtraction, so the derivative keeps its relative accuracy
// at |x| = 12, where o rounds to within 6e-8 of 1.
S3O_HD void sigmoid_and_slope(float x, float& o, float& slope) {
  const float e = expf(-fabsf(x));
  const float d = 1.0f + e;
  o = (x >= 0.0f ? 1.0f : e) / d;
  slope = e / (d * d);
}

// Unit quaternion and the norm it was divided by, for the chain rule.  A
// quaternion whose float32 norm is zero, NaN or overflows to +Inf gives the
// identity and nn = 0 (and so a zero gradient).
S3O_HD void unit_quat(const float (&r)[kRow], float (&q)[4], float& nn) {
  const float w = r[10], x = r[11], y = r[12], z = r[13];
  nn = sqrtf(w * w + x * x + y * y + z * z);
  if (nn > 0.0f && nn <= 3.402823466e+38f) {
    q[0] = w / nn; q[1] = x / nn; q[2] = y / nn; q[3] = z / nn;
  } else {
    nn = 0.0f;
    q[0] = 1.0f; q[1] = q[2] = q[3] = 0.0f;
  }
}

// The five tensors the rasterizer takes, from one row.  The transcendental
// and the normalised outputs are formed in double and rounded to float32
// once, so each is the float32 nearest the exact value (the float32 product
// s * x already is): a float64 activation of the same row, cast to float32,
// feeds the rasterizer the same bits.  One ulp matters there: the photometric
// backward turns a 1.8e-7 change of the image into a 1e-5 relative change of
// dL/dimage.  The kernel is bound by its 112 bytes per row,
// not by this arithmetic.
S3O_HD void activate(const float (&r)[kRow], float s, float (&mean)[3], float (&sh)[3],
                     float& opacity, float (&scale)[3], float (&q)[4]) {
  const double sd = (double)s;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mean[k] = s * r[k];
    sh[k] = r[3 + k];
    scale[k] = (float)(sd * exp((double)r[7 + k]));
  }
  const double e = exp(-fabs((double)r[6]));
  opacity = (float)((r[6] >= 0.0f ? 1.0 : e) / (1.0 + e));
  const double w = r[10], x = r[11], y = r[12], z = r[13];
  const double nn = sqrt(w * w + x * x + y * y + z * z);  // cannot overflow in double
  if (nn > 0.0) {
    q[0] = (float)(w / nn); q[1] = (float)(x / nn); q[2] = (float)(y / nn);
    q[3] = (float)(z / nn);
  } else {
    q[0] = 1.0f; q[1] = q[2] = q[3] = 0.0f;
  }
}

// Gradient of the row, g[14], from the gradients of the activated tensors.
// The activations needed are recomputed from the row.
S3O_HD void row_grad(const float (&r)[kRow], float s, const float (&dmean)[3],
                     const float (&dsh)[3], float dop, const float (&dscale)[3],
                     const float (&dq)[4], float (&g)[kRow]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g[k] = s * dmean[k];
    g[3 + k] = dsh[k];
    g[7 + k] = dscale[k] * (s * expf(r[7 + k]));
  }
  float o, slope;
  sigmoid_and_slope(r[6], o, slope);
  g[6] = dop * slope;
  float q[4], nn;
  unit_quat(r, q, nn);
  const float dot = q[0] * dq[0] + q[1] * dq[1] + q[2] * dq[2] + q[3] * dq[3];
  const bool live = nn > 0.0f;
  const float den = live ? nn : 1.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) g[10 + k] = live ? (dq[k] - q[k] * dot) / den : 0.0f;
}

// One Adam update of one scalar.  step = lr / (1 - beta1^t), bias2_sqrt =
// sqrt(1 - beta2^t); 1 - beta is exact in float32 for beta in [0.5, 1].
// The first moment is written as torch writes it (lerp): m + (1 - beta1)
// (g - m) is beta1 m + (1 - beta1) g without the cancellation of two rounded
// products when g and m have opposite signs.
S3O_HD void adam_update(float& p, float& m, float& v, float g, float step, float beta1,
                        float beta2, float eps, float bias2_sqrt) {
  m = m + (1.0f - beta1) * (g - m);
  v = beta2 * v + (1.0f - beta2) * (g * g);
  p = p - step * (m / (sqrtf(v) / bias2_sqrt + eps));
}

// All 14 entries finite?
S3O_HD bool all_finite(const float (&dmean)[3], const float (&dsh)[3], float dop,
                       const float (&dscale)[3], const float (&dq)[4]) {
  bool ok = fabsf(dop) <= 3.402823466e+38f;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    ok = ok && fabsf(dmean[k]) <= 3.402823466e+38f && fabsf(dsh[k]) <= 3.402823466e+38f &&
         fabsf(dscale[k]) <= 3.402823466e+38f;
#pragma unroll
  for (int k = 0; k < 4; ++k) ok = ok && fabsf(dq[k]) <= 3.402823466e+38f;
  return ok;
}

// The fused step of one row: chain rule, then Adam on its 14 entries.
// lr[5], by group; the rest as in s3o_adam (include/s3o.h).
S3O_HD void adam_row(float (&r)[kRow], float (&m)[kRow], float (&v)[kRow], float s,
                     const float (&dmean)[3], const float (&dsh)[3], float dop,
                     const float (&dscale)[3], const float (&dq)[4], const float (&lr)[kGroups],
                     float beta1, float beta2, float eps, float bias1, float bias2_sqrt) {
  float g[kRow];
  row_grad(r, s, dmean, dsh, dop, dscale, dq, g);
  float step[kGroups];
#pragma unroll
  for (int k = 0; k < kGroups; ++k) step[k] = lr[k] / bias1;
#pragma unroll
  for (int k = 0; k < kRow; ++k)
    adam_update(r[k], m[k], v[k], g[k], step[group_of(k)], beta1, beta2, eps, bias2_sqrt);
}

}  // namespace s3o
