// Arithmetic of the pose gradient and the pose step (pose_grad.hip,
// include/s3x.h s3x_pose_grad / s3x_pose_step), host + device so a host
// program can restate it (tests/native/pose_grad_host.cpp).  Everything is
// double: the reduction is bound by the 60..76 bytes it loads per row, not by
// this arithmetic, and the step is one thread.
//
// Moving the camera by T_WC <- T_WC Exp(xi), xi = (rho, phi), moves a
// view-space point t to Exp(-xi) t: to first order by -(rho + phi x t), and
// turns a view-space covariance S_v into Rd S_v Rd^T with Rd = exp(-[phi]x).
// With A = vm[:3,:3]^T, b = vm[3,:3] (t = A mu + b), g = A^-T dL/dmu:
//   dL/drho = -sum g,  dL/dphi = -sum (t x g + c)
//   c = 2 axial(G_v S_v - S_v G_v)            (covariance given)
//   c = R_c w, w = 1/2 (q_r dq_v - dq_r q_v + q_v x dq_v)   (unit quaternion)
// Build with -ffp-contract=off: every product and sum rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define S3X_HD __host__ __device__ __forceinline__

namespace s3x {

// What a row's contribution needs of the view matrix.
struct Cam {
  double A[9];    // row-major, t = A mu + b
  double b[3];
  double Ait[9];  // A^-T
  double Rc[9];   // A / cbrt(det A): the rotation of a scaled rotation
};

S3X_HD void cam_from_view(const float* vm, Cam& c) {
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) c.A[3 * r + k] = (double)vm[4 * k + r];
    c.b[r] = (double)vm[12 + r];
  }
  const double* A = c.A;
  // cofactors: A^-T = cof(A) / det A
  double cof[9];
  cof[0] = A[4] * A[8] - A[5] * A[7];
  cof[1] = A[5] * A[6] - A[3] * A[8];
  cof[2] = A[3] * A[7] - A[4] * A[6];
  cof[3] = A[2] * A[7] - A[1] * A[8];
  cof[4] = A[0] * A[8] - A[2] * A[6];
  cof[5] = A[1] * A[6] - A[0] * A[7];
  cof[6] = A[1] * A[5] - A[2] * A[4];
  cof[7] = A[2] * A[3] - A[0] * A[5];
  cof[8] = A[0] * A[4] - A[1] * A[3];
  const double det = A[0] * cof[0] + A[1] * cof[1] + A[2] * cof[2];
  const double s = cbrt(det);
  for (int k = 0; k < 9; ++k) {
    c.Ait[k] = cof[k] / det;
    c.Rc[k] = A[k] / s;
  }
}

S3X_HD bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }

S3X_HD void mat_vec(const double* M, const double* x, double* y) {
  for (int r = 0; r < 3; ++r) y[r] = M[3 * r] * x[0] + M[3 * r + 1] * x[1] + M[3 * r + 2] * x[2];
}

// C = X Y (3 x 3, row-major)
S3X_HD void mat_mul(const double* X, const double* Y, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k)
      C[3 * r + k] = X[3 * r] * Y[k] + X[3 * r + 1] * Y[3 + k] + X[3 * r + 2] * Y[6 + k];
}

// C = X Y^T
S3X_HD void mat_mul_t(const double* X, const double* Y, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k)
      C[3 * r + k] = X[3 * r] * Y[3 * k] + X[3 * r + 1] * Y[3 * k + 1] + X[3 * r + 2] * Y[3 * k + 2];
}

// The part every row shares: acc[0..2] -= g, acc[3..5] -= t x g.
S3X_HD void sub_mean_term(const Cam& c, const float (&mu)[3], const float (&dmu)[3],
                          double (&acc)[6]) {
  const double m[3] = {(double)mu[0], (double)mu[1], (double)mu[2]};
  const double d[3] = {(double)dmu[0], (double)dmu[1], (double)dmu[2]};
  double t[3], g[3];
  mat_vec(c.A, m, t);
  for (int k = 0; k < 3; ++k) t[k] = t[k] + c.b[k];
  mat_vec(c.Ait, d, g);
  acc[0] -= g[0];
  acc[1] -= g[1];
  acc[2] -= g[2];
  acc[3] -= t[1] * g[2] - t[2] * g[1];
  acc[4] -= t[2] * g[0] - t[0] * g[2];
  acc[5] -= t[0] * g[1] - t[1] * g[0];
}

// One row, covariance given.  false (and acc untouched): a non-finite input.
S3X_HD bool sub_row_cov(const Cam& c, const float (&mu)[3], const float (&dmu)[3],
                        const float (&cov)[6], const float (&dcov)[6], double (&acc)[6]) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && finite_f(mu[k]) && finite_f(dmu[k]);
  for (int k = 0; k < 6; ++k) ok = ok && finite_f(cov[k]) && finite_f(dcov[k]);
  if (!ok) return false;
  sub_mean_term(c, mu, dmu, acc);
  const double S[9] = {(double)cov[0], (double)cov[1], (double)cov[2],
                       (double)cov[1], (double)cov[3], (double)cov[4],
                       (double)cov[2], (double)cov[4], (double)cov[5]};
  const double G[9] = {(double)dcov[0],       0.5 * (double)dcov[1], 0.5 * (double)dcov[2],
                       0.5 * (double)dcov[1], (double)dcov[3],       0.5 * (double)dcov[4],
                       0.5 * (double)dcov[2], 0.5 * (double)dcov[4], (double)dcov[5]};
  double T[9], Sv[9], Gv[9], M[9];
  mat_mul(c.A, S, T);
  mat_mul_t(T, c.A, Sv);      // A S A^T
  mat_mul(c.Ait, G, T);
  mat_mul_t(T, c.Ait, Gv);    // A^-T G A^-1
  mat_mul(Gv, Sv, M);         // G_v S_v; S_v G_v is its transpose
  acc[3] -= 2.0 * (M[7] - M[5]);
  acc[4] -= 2.0 * (M[2] - M[6]);
  acc[5] -= 2.0 * (M[3] - M[1]);
  return true;
}

// One row, unit quaternion (r, x, y, z) given.
S3X_HD bool sub_row_rot(const Cam& c, const float (&mu)[3], const float (&dmu)[3],
                        const float (&q)[4], const float (&dq)[4], double (&acc)[6]) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && finite_f(mu[k]) && finite_f(dmu[k]);
  for (int k = 0; k < 4; ++k) ok = ok && finite_f(q[k]) && finite_f(dq[k]);
  if (!ok) return false;
  sub_mean_term(c, mu, dmu, acc);
  const double qr = q[0], qx = q[1], qy = q[2], qz = q[3];
  const double dr = dq[0], dx = dq[1], dy = dq[2], dz = dq[3];
  const double w[3] = {0.5 * (qr * dx - dr * qx + (qy * dz - qz * dy)),
                       0.5 * (qr * dy - dr * qy + (qz * dx - qx * dz)),
                       0.5 * (qr * dz - dr * qz + (qx * dy - qy * dx))};
  double cw[3];
  mat_vec(c.Rc, w, cw);
  acc[3] -= cw[0];
  acc[4] -= cw[1];
  acc[5] -= cw[2];
  return true;
}

// ------------------------------------------------------------ the pose step
// SE(3) Exp of (rho, phi): R [9] and p = V rho.  With th = |phi| and K = [phi]x:
//   R = I + a K + b K^2, V = I + b K + c K^2,
//   a = sin th / th, b = (1 - cos th) / th^2 = 1/2 (sin(th/2) / (th/2))^2,
//   c = (th - sin th) / th^3, a series below th = 0.5 (the closed form cancels
//   there; eight terms leave 1e-18).
S3X_HD void se3_exp(const double (&xi)[6], double (&R)[9], double (&p)[3]) {
  const double x = xi[3], y = xi[4], z = xi[5];
  const double t2 = x * x + y * y + z * z;
  const double th = sqrt(t2);
  double a, b, c;
  if (th > 0.0) {
    a = sin(th) / th;
    const double h = sin(0.5 * th) / (0.5 * th);
    b = 0.5 * h * h;
  } else {
    a = 1.0;
    b = 0.5;
  }
  if (th < 0.5) {
    // sum_k (-t2)^k / (2k + 3)!, Horner from k = 7
    c = 1.0 / 355687428096000.0;                    // 1 / 17!
    c = 1.0 / 1307674368000.0 - t2 * c;             // 1 / 15!
    c = 1.0 / 6227020800.0 - t2 * c;                // 1 / 13!
    c = 1.0 / 39916800.0 - t2 * c;                  // 1 / 11!
    c = 1.0 / 362880.0 - t2 * c;                    // 1 / 9!
    c = 1.0 / 5040.0 - t2 * c;                      // 1 / 7!
    c = 1.0 / 120.0 - t2 * c;                       // 1 / 5!
    c = 1.0 / 6.0 - t2 * c;                         // 1 / 3!
  } else {
    c = (th - sin(th)) / (t2 * th);
  }
  const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
  double K2[9];
  mat_mul(K, K, K2);
  double V[9];
  for (int k = 0; k < 9; ++k) {
    const double e = (k % 4 == 0) ? 1.0 : 0.0;
    R[k] = e + (a * K[k] + b * K2[k]);
    V[k] = e + (b * K[k] + c * K2[k]);
  }
  const double rho[3] = {xi[0], xi[1], xi[2]};
  mat_vec(V, rho, p);
}

struct PoseAdam {
  double lr_translation, lr_rotation, beta1, beta2, eps, bias1, bias2_sqrt, render_scale;
};

// Adam on the six twist components, then T <- T Exp(-delta).  T [16]
// row-major (s R | t).  false, and nothing written: a non-finite gradient.
S3X_HD bool pose_step(double (&T)[16], double (&m)[6], double (&v)[6], const double (&grad)[6],
                      const PoseAdam& hp) {
  for (int k = 0; k < 6; ++k)
    if (!(fabs(grad[k]) <= 1.7976931348623157e308)) return false;
  double xi[6];
  for (int k = 0; k < 6; ++k) {
    const double g = k < 3 ? hp.render_scale * grad[k] : grad[k];
    const double lr = k < 3 ? hp.lr_translation : hp.lr_rotation;
    m[k] = m[k] + (1.0 - hp.beta1) * (g - m[k]);
    v[k] = hp.beta2 * v[k] + (1.0 - hp.beta2) * (g * g);
    xi[k] = -((lr / hp.bias1) * (m[k] / (sqrt(v[k]) / hp.bias2_sqrt + hp.eps)));
  }
  double R[9], p[3];
  se3_exp(xi, R, p);
  double B[9], N[9], dt[3];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) B[3 * r + k] = T[4 * r + k];
  mat_mul(B, R, N);
  mat_vec(B, p, dt);
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) T[4 * r + k] = N[3 * r + k];
    T[4 * r + 3] = T[4 * r + 3] + dt[r];
  }
  return true;
}

// The float32 camera of a pose: ext = T with its translation times
// render_scale; view = (ext^-1)^T, full = view @ proj_t, campos = ext[:3,3].
S3X_HD void pose_camera(const double (&T)[16], double render_scale, const float* proj_t,
                        float* view, float* full, float* campos) {
  double B[9], ts[3];
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) B[3 * r + k] = T[4 * r + k];
    ts[r] = render_scale * T[4 * r + 3];
  }
  // inverse of the 3 x 3 block by cofactors; inv[r][k] = cof[k][r] / det
  double cof[9];
  cof[0] = B[4] * B[8] - B[5] * B[7];
  cof[1] = B[5] * B[6] - B[3] * B[8];
  cof[2] = B[3] * B[7] - B[4] * B[6];
  cof[3] = B[2] * B[7] - B[1] * B[8];
  cof[4] = B[0] * B[8] - B[2] * B[6];
  cof[5] = B[1] * B[6] - B[0] * B[7];
  cof[6] = B[1] * B[5] - B[2] * B[4];
  cof[7] = B[2] * B[3] - B[0] * B[5];
  cof[8] = B[0] * B[4] - B[1] * B[3];
  const double det = B[0] * cof[0] + B[1] * cof[1] + B[2] * cof[2];
  // V = (ext^-1)^T: V[r][k] = inv[k][r] = cof[r][k] / det for the block,
  // row 3 = -(inv ts)
  double V[16];
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) V[4 * r + k] = cof[3 * r + k] / det;
    V[4 * r + 3] = 0.0;
  }
  for (int k = 0; k < 3; ++k)
    V[12 + k] = -(V[k] * ts[0] + V[4 + k] * ts[1] + V[8 + k] * ts[2]);
  V[15] = 1.0;
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 4; ++k) {
      double s = 0.0;
      for (int j = 0; j < 4; ++j) s += V[4 * r + j] * (double)proj_t[4 * j + k];
      full[4 * r + k] = (float)s;
      view[4 * r + k] = (float)V[4 * r + k];
    }
  for (int r = 0; r < 3; ++r) campos[r] = (float)ts[r];
}

}  // namespace s3x
