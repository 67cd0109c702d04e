// Per-Gaussian arithmetic of the splat-file export and import (splat_io.hip,
// include/s3w.h s3w_map_to_splats / s3w_map_from_splats), host + device so a
// host program can restate it (tests/native/splat_rows_host.cpp).
//
// Export: covariance (packed triu) -> three log-scales (descending) and the
// unit quaternion (w, x, y, z; w >= 0) of the proper rotation whose columns
// are the eigenvectors in the same order.  The eigendecomposition is a cyclic
// Jacobi iteration on the matrix divided by its largest |entry|, a fixed
// number of sweeps with no convergence test: the result of one Gaussian
// depends on nothing but its own six numbers.
// Build with -ffp-contract=off: every product and sum rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define S3W_HD __host__ __device__ __forceinline__

namespace s3w {

constexpr float kC0 = 0.28209479177387814f;
constexpr int kRowFloats = 17;    // x y z nx ny nz f_dc[3] opacity scale[3] rot[4]
constexpr int kRow14Floats = 14;  // x y z f_dc[3] opacity scale[3] rot[4]
static_assert(kRow14Floats % 2 == 0, "a 14-float row is whole float2s");
// Cyclic Jacobi converges quadratically once the off-diagonal part is small:
// float32 3x3 matrices are converged after 4 sweeps (errors against float64
// no longer change), the fifth is margin.  The kernel takes
// longer than its bytes need, so sweeps are not free.
#ifndef S3W_JACOBI_SWEEPS
#define S3W_JACOBI_SWEEPS 5
#endif
constexpr int kJacobiSweeps = S3W_JACOBI_SWEEPS;

// One Jacobi rotation in the (p, q) plane; r is the third index.  a: the
// symmetric matrix as a[3][3] (both triangles kept), v: eigenvector columns.
S3W_HD void jacobi_rotate(float (&a)[3][3], float (&v)[3][3], int p, int q, int r) {
  const float apq = a[p][q];
  // tan of the rotation angle, the smaller root of t^2 + 2 t theta - 1 = 0
  // with theta = d / (2 apq), d = aqq - app, written with one division:
  //   t = sign(d) 2 apq / (|d| + sqrt(d^2 + 4 apq^2)).
  // The matrix is scaled to entries <= 1, so nothing overflows; every term of
  // the denominator is >= 0, so nothing cancels.  d = 0 gives t = +-1 (45
  // degrees).  A zero denominator (apq = 0, or d = 0 and apq^2 underflowing)
  // takes t = 0: the entry dropped is below 1e-19 of the largest.
  const float d = a[q][q] - a[p][p];
  const float b = 2.0f * apq;
  const float den = fabsf(d) + sqrtf(d * d + b * b);
  const float t = (den > 0.0f) ? copysignf(b, d * b) / den : 0.0f;
  const float c = 1.0f / sqrtf(t * t + 1.0f);
  const float s = t * c;
  a[p][p] = a[p][p] - t * apq;
  a[q][q] = a[q][q] + t * apq;
  a[p][q] = a[q][p] = 0.0f;
  const float arp = a[r][p], arq = a[r][q];
  a[r][p] = a[p][r] = c * arp - s * arq;
  a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float vkp = v[k][p], vkq = v[k][q];
    v[k][p] = c * vkp - s * vkq;
    v[k][q] = s * vkp + c * vkq;
  }
}

// Swap eigenpairs i and j when lam[i] < lam[j] (descending order).
S3W_HD void order_pair(float (&lam)[3], float (&v)[3][3], int i, int j) {
  const bool sw = lam[i] < lam[j];
  const float li = lam[i], lj = lam[j];
  lam[i] = sw ? lj : li;
  lam[j] = sw ? li : lj;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = v[k][i], b = v[k][j];
    v[k][i] = sw ? b : a;
    v[k][j] = sw ? a : b;
  }
}

// Proper rotation (columns of R) -> unit quaternion (w, x, y, z), w >= 0, by
// the branch on the largest of (trace, R00, R11, R22).
S3W_HD void rotation_to_quat(const float (&R)[3][3], float& qw, float& qx, float& qy,
                             float& qz) {
  const float tr = R[0][0] + R[1][1] + R[2][2];
  float w, x, y, z;
  if (tr >= R[0][0] && tr >= R[1][1] && tr >= R[2][2]) {
    const float s = 2.0f * sqrtf(fmaxf(1.0f + tr, 0.0f));
    w = 0.25f * s;
    x = (R[2][1] - R[1][2]) / s;
    y = (R[0][2] - R[2][0]) / s;
    z = (R[1][0] - R[0][1]) / s;
  } else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) {
    const float s = 2.0f * sqrtf(fmaxf(1.0f + R[0][0] - R[1][1] - R[2][2], 0.0f));
    w = (R[2][1] - R[1][2]) / s;
    x = 0.25f * s;
    y = (R[0][1] + R[1][0]) / s;
    z = (R[0][2] + R[2][0]) / s;
  } else if (R[1][1] >= R[2][2]) {
    const float s = 2.0f * sqrtf(fmaxf(1.0f + R[1][1] - R[0][0] - R[2][2], 0.0f));
    w = (R[0][2] - R[2][0]) / s;
    x = (R[0][1] + R[1][0]) / s;
    y = 0.25f * s;
    z = (R[1][2] + R[2][1]) / s;
  } else {
    const float s = 2.0f * sqrtf(fmaxf(1.0f + R[2][2] - R[0][0] - R[1][1], 0.0f));
    w = (R[1][0] - R[0][1]) / s;
    x = (R[0][2] + R[2][0]) / s;
    y = (R[1][2] + R[2][1]) / s;
    z = 0.25f * s;
  }
  // the largest of the four branch quantities of a rotation is >= 0, so
  // s >= 2 and the norm below is ~1: the division only removes the 1e-7
  // loss of orthogonality the sweeps leave
  const float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
  const float sg = (w < 0.0f) ? -inv : inv;
  qw = w * sg;
  qx = x * sg;
  qy = y * sg;
  qz = z * sg;
}

// cov: xx xy xz yy yz zz.  scale[i] = log(max(sqrt(max(lambda_i, 0)),
// scale_min)), lambda descending.  A zero (or non-finite) matrix gives
// scale_min three times and the identity quaternion.
S3W_HD void cov_to_scale_rot(const float (&cov)[6], float scale_min, float (&scale)[3],
                             float (&q)[4]) {
  float m = 0.0f;
#pragma unroll
  for (int k = 0; k < 6; ++k) m = fmaxf(m, fabsf(cov[k]));
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) finite = finite && (fabsf(cov[k]) <= 3.402823466e+38f);
  // no early return: the degenerate case runs the same instructions on a
  // stand-in divisor and is selected at the end
  const bool degenerate = !(m > 0.0f) || !finite;
  m = degenerate ? 1.0f : m;
  float a[3][3], v[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
  a[0][0] = cov[0] / m;
  a[0][1] = a[1][0] = cov[1] / m;
  a[0][2] = a[2][0] = cov[2] / m;
  a[1][1] = cov[3] / m;
  a[1][2] = a[2][1] = cov[4] / m;
  a[2][2] = cov[5] / m;
#pragma unroll 1
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate(a, v, 0, 1, 2);
    jacobi_rotate(a, v, 0, 2, 1);
    jacobi_rotate(a, v, 1, 2, 0);
  }
  float lam[3] = {a[0][0], a[1][1], a[2][2]};
  order_pair(lam, v, 0, 1);
  order_pair(lam, v, 0, 2);
  order_pair(lam, v, 1, 2);
  // det(v) = v0 . (v1 x v2); a reflection flips the third column
  const float det = v[0][0] * (v[1][1] * v[2][2] - v[2][1] * v[1][2]) -
                    v[1][0] * (v[0][1] * v[2][2] - v[2][1] * v[0][2]) +
                    v[2][0] * (v[0][1] * v[1][2] - v[1][1] * v[0][2]);
  if (det < 0.0f) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k][2] = -v[k][2];
  }
  const float sqrt_m = sqrtf(m);
  // written out, not a loop over k: one that is not unrolled would index
  // lam and scale at run time and put them in scratch memory
  const float e0 = fmaxf(sqrtf(fmaxf(lam[0], 0.0f)) * sqrt_m, scale_min);
  const float e1 = fmaxf(sqrtf(fmaxf(lam[1], 0.0f)) * sqrt_m, scale_min);
  const float e2 = fmaxf(sqrtf(fmaxf(lam[2], 0.0f)) * sqrt_m, scale_min);
  scale[0] = logf(degenerate ? scale_min : e0);
  scale[1] = logf(degenerate ? scale_min : e1);
  scale[2] = logf(degenerate ? scale_min : e2);
  float qw, qx, qy, qz;
  rotation_to_quat(v, qw, qx, qy, qz);
  q[0] = degenerate ? 1.0f : qw;
  q[1] = degenerate ? 0.0f : qx;
  q[2] = degenerate ? 0.0f : qy;
  q[3] = degenerate ? 0.0f : qz;
}

// One 17-float export row.
S3W_HD void splat_row(const float (&mean)[3], const float (&cov)[6], const float (&color)[3],
                      float opacity, float scale_min, float (&row)[kRowFloats]) {
  row[0] = mean[0];
  row[1] = mean[1];
  row[2] = mean[2];
  row[3] = row[4] = row[5] = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) row[6 + k] = (color[k] - 0.5f) / kC0;
  const float o = fminf(fmaxf(opacity, 1e-6f), 1.0f - 1e-6f);
  row[9] = logf(o / (1.0f - o));
  float scale[3], q[4];
  cov_to_scale_rot(cov, scale_min, scale, q);
#pragma unroll
  for (int k = 0; k < 3; ++k) row[10 + k] = scale[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) row[13 + k] = q[k];
}

// One import row (14 floats) -> the map's fields.  The quaternion is
// normalised first (INRIA files store it raw); a zero quaternion is the
// identity.
S3W_HD void splat_unpack(const float (&r)[kRow14Floats], float (&mean)[3], float (&cov)[6],
                         float (&color)[3], float& opacity) {
  mean[0] = r[0];
  mean[1] = r[1];
  mean[2] = r[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) color[k] = fminf(fmaxf(r[3 + k] * kC0 + 0.5f, 0.0f), 1.0f);
  opacity = 1.0f / (1.0f + expf(-r[6]));
  float w = r[10], x = r[11], y = r[12], z = r[13];
  const float nn = sqrtf(w * w + x * x + y * y + z * z);
  if (nn > 0.0f) {
    w = w / nn; x = x / nn; y = y / nn; z = z / nn;
  } else {
    w = 1.0f; x = y = z = 0.0f;
  }
  const float R[3][3] = {
      {1.f - 2.f * (y * y + z * z), 2.f * (x * y - w * z), 2.f * (x * z + w * y)},
      {2.f * (x * y + w * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - w * x)},
      {2.f * (x * z - w * y), 2.f * (y * z + w * x), 1.f - 2.f * (x * x + y * y)}};
  // M = R diag(exp(scale)); cov = M M^T
  float M[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float s = expf(r[7 + j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) M[i][j] = R[i][j] * s;
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j)
      cov[k++] = M[i][0] * M[j][0] + M[i][1] * M[j][1] + M[i][2] * M[j][2];
}

// A 14-float row as seven 8-byte accesses (rows are 56 B: 8-byte aligned).
__device__ __forceinline__ void load_row(const float* __restrict__ base, int64_t i,
                                         float (&r)[kRow14Floats]) {
  const float2* p = reinterpret_cast<const float2*>(base + i * kRow14Floats);
#pragma unroll
  for (int k = 0; k < kRow14Floats / 2; ++k) {
    const float2 t = p[k];
    r[2 * k] = t.x;
    r[2 * k + 1] = t.y;
  }
}

__device__ __forceinline__ void store_row(float* __restrict__ base, int64_t i,
                                          const float (&r)[kRow14Floats]) {
  float2* p = reinterpret_cast<float2*>(base + i * kRow14Floats);
#pragma unroll
  for (int k = 0; k < kRow14Floats / 2; ++k) p[k] = make_float2(r[2 * k], r[2 * k + 1]);
}

__device__ __forceinline__ void zero_row(float* __restrict__ base, int64_t i) {
  float2* p = reinterpret_cast<float2*>(base + i * kRow14Floats);
#pragma unroll
  for (int k = 0; k < kRow14Floats / 2; ++k) p[k] = make_float2(0.0f, 0.0f);
}

}  // namespace s3w
