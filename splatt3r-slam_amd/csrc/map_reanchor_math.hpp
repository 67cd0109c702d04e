// Per-keyframe and per-Gaussian arithmetic of the map re-anchor
// (map_reanchor.hip, include/s3a.h), host + device so a host program can
// restate it (tests/native/map_reanchor_host.cpp).
//
// A pose row is lietorch's [t(3), q(x y z w), s] in float32.  Everything here
// is double on the float32 inputs; each output is rounded to float32 once.
// Build with -ffp-contract=off: every product and sum rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#define S3A_HD __host__ __device__ __forceinline__

namespace s3a {

constexpr int kPose = 8;     // floats of a pose row
constexpr int kDelta = 16;   // doubles of a keyframe's delta: flag, M[9], t_o[3], t_n[3]
enum : int { kKeep = 0, kMove = 1 };

S3A_HD bool finite32(float v) { return fabsf(v) <= 3.402823466e+38f; }

// |q| in double: the squares of float32 values neither overflow nor vanish.
S3A_HD double quat_norm(const float* p) {
  const double x = p[3], y = p[4], z = p[5], w = p[6];
  return sqrt(x * x + y * y + z * z + w * w);
}

// 8 finite entries, s > 0, |q| > 0.
S3A_HD bool pose_valid(const float* p) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kPose; ++k) ok = ok && finite32(p[k]);
  return ok && p[7] > 0.0f && quat_norm(p) > 0.0;
}

// Equal in all eight 32-bit patterns (-0 != +0, a NaN equals itself).
S3A_HD bool pose_same_bits(const float* a, const float* b) {
  bool same = true;
#pragma unroll
  for (int k = 0; k < kPose; ++k) {
    uint32_t ua, ub;
    memcpy(&ua, a + k, 4);
    memcpy(&ub, b + k, 4);
    same = same && ua == ub;
  }
  return same;
}

// Row-major rotation of the pose's quaternion, normalised in double.
S3A_HD void rotation(const float* p, double (&R)[9]) {
  const double nn = quat_norm(p);
  const double x = p[3] / nn, y = p[4] / nn, z = p[5] / nn, w = p[6] / nn;
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - z * w);
  R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w);
  R[7] = 2.0 * (y * z + x * w);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// Classify keyframe k (include/s3a.h) and fill its delta.  Returns true when
// the keyframe is held; `adopt` says whether anchor := pose afterwards.
S3A_HD bool classify(const float* anchor, const float* pose, double (&d)[kDelta], bool& adopt) {
  d[0] = (double)kKeep;
#pragma unroll
  for (int k = 1; k < kDelta; ++k) d[k] = 0.0;
  adopt = false;
  if (!pose_valid(pose)) return true;
  adopt = true;
  if (anchor[7] == 0.0f || !pose_valid(anchor)) return false;   // unset: adopt, move nothing
  if (pose_same_bits(anchor, pose)) return false;
  double Rn[9], Ro[9];
  rotation(pose, Rn);
  rotation(anchor, Ro);
  const double s = (double)pose[7] / (double)anchor[7];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      d[1 + i * 3 + j] =
          s * (Rn[i * 3 + 0] * Ro[j * 3 + 0] + Rn[i * 3 + 1] * Ro[j * 3 + 1] +
               Rn[i * 3 + 2] * Ro[j * 3 + 2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[10 + k] = (double)anchor[k];
    d[13 + k] = (double)pose[k];
  }
  d[0] = (double)kMove;
  return false;
}

// One Gaussian under a delta's M = d[1..9], t_o = d[10..12], t_n = d[13..15]:
// mu' = t_n + M (mu - t_o), Sigma' = M Sigma M^T (c6 = xx xy xz yy yz zz).
S3A_HD void move_row(const double* d, float (&mu)[3], float (&c6)[6]) {
  const double* M = d + 1;
  const double e[3] = {(double)mu[0] - d[10], (double)mu[1] - d[11], (double)mu[2] - d[12]};
#pragma unroll
  for (int i = 0; i < 3; ++i)
    mu[i] = (float)(d[13 + i] + (M[i * 3 + 0] * e[0] + M[i * 3 + 1] * e[1] + M[i * 3 + 2] * e[2]));
  const double S[9] = {c6[0], c6[1], c6[2], c6[1], c6[3], c6[4], c6[2], c6[4], c6[5]};
  double A[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l)
      A[i * 3 + l] = M[i * 3 + 0] * S[0 * 3 + l] + M[i * 3 + 1] * S[1 * 3 + l] +
                     M[i * 3 + 2] * S[2 * 3 + l];
  int o = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j)
      c6[o++] = (float)(A[i * 3 + 0] * M[j * 3 + 0] + A[i * 3 + 1] * M[j * 3 + 1] +
                        A[i * 3 + 2] * M[j * 3 + 2]);
}

}  // namespace s3a
