// Per-pixel arithmetic of the depth loss and depth-metric sums
// (depth_loss.hip, include/s3z.h), host + device so a host program can restate
// it (tests/native/depth_loss_host.cpp).
//
// pixel()       validity, w, q, p, r of one pixel
// terms()       the pixel's addends of the per-pixel sums
// pair_weight(), pair_term()   one pair's addends of S3Z_SUM_WG / S3Z_SUM_GRAD
// dl_dr()       dL/dr of a pixel from its own (w, r) and its four neighbours'
// grads()       dL/dD, dL/dA from dL/dr
// Build with -ffp-contract=off: every operation rounds once, in double.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "s3z.h"

#define S3Z_HD __host__ __device__ __forceinline__

namespace s3z {

constexpr double kDblMax = 1.7976931348623157e308;
constexpr double kDelta1 = 1.25, kDelta2 = 1.5625, kDelta3 = 1.953125;   // 1.25^k, exact

// w == 0 marks an invalid pixel (a valid one has w > 0); r is 0 there
struct Pixel {
  double w, q, p, r;
};

S3Z_HD bool finite(double x) { return fabs(x) <= kDblMax; }

S3Z_HD double sign(double x) { return (double)((x > 0.0) - (x < 0.0)); }

// s: the image's scale (1 without one); wf: the pixel's weight (1 without one)
S3Z_HD Pixel pixel(float Df, float Af, float zf, float wf, double s, double alpha_min) {
  const double D = (double)Df, A = (double)Af, z = (double)zf, w = (double)wf;
  Pixel px{0.0, 0.0, 0.0, 0.0};
  const bool ok = finite(z) && z > 0.0 && finite(D) && finite(A) && D > 0.0 && A > 0.0 &&
                  A >= alpha_min && finite(w) && w > 0.0 && finite(s) && s > 0.0;
  if (ok) {
    px.w = w;
    px.q = D / A;
    px.p = s * px.q;
    px.r = px.p - z;
  }
  return px;
}

// the addends of a valid pixel; t[S3Z_SUM_GRAD] and t[S3Z_SUM_WG] are the pairs'
S3Z_HD void terms(const Pixel& px, float zf, double (&t)[S3Z_NSUMS]) {
  const double z = (double)zf;
  const double a = fabs(px.r);
  const double wa = px.w * a;
  const double waa = wa * a;
  const double l = log(px.p) - log(z);
  const double up = px.p / z, down = z / px.p;
  const double ratio = up > down ? up : down;
  const double wq = px.w * px.q;
  t[S3Z_SUM_W] = px.w;
  t[S3Z_SUM_ABS] = wa;
  t[S3Z_SUM_SQ] = waa;
  t[S3Z_SUM_ABSREL] = wa / z;
  t[S3Z_SUM_SQREL] = waa / z;
  t[S3Z_SUM_LOGSQ] = px.w * (l * l);
  t[S3Z_SUM_GRAD] = 0.0;
  t[S3Z_SUM_WG] = 0.0;
  t[S3Z_SUM_D1] = ratio < kDelta1 ? 1.0 : 0.0;
  t[S3Z_SUM_D2] = ratio < kDelta2 ? 1.0 : 0.0;
  t[S3Z_SUM_D3] = ratio < kDelta3 ? 1.0 : 0.0;
  t[S3Z_SUM_N] = 1.0;
  t[S3Z_SUM_QZ] = wq * z;
  t[S3Z_SUM_QQ] = wq * px.q;
}

// a pair of two valid pixels
S3Z_HD double pair_weight(double wp, double wq) { return 0.5 * (wp + wq); }

S3Z_HD double pair_term(double wp, double rp, double wq, double rq) {
  return pair_weight(wp, wq) * fabs(rq - rp);
}

// one neighbour's share of dL/dr_p / c_grad; 0 when the neighbour is invalid (wq == 0)
S3Z_HD double pair_sign(double wp, double rp, double wq, double rq) {
  return wq > 0.0 ? pair_weight(wp, wq) * sign(rp - rq) : 0.0;
}

// dL/dr of a valid pixel; neighbours in the order left, right, up, down,
// each (w, r) with w == 0 where there is none
S3Z_HD double dl_dr(double w, double r, double wl, double rl, double wr, double rr, double wu,
                    double ru, double wd, double rd, double c_abs, double c_sq, double c_grad) {
  const double g = ((pair_sign(w, r, wl, rl) + pair_sign(w, r, wr, rr)) +
                    pair_sign(w, r, wu, ru)) + pair_sign(w, r, wd, rd);
  return w * (c_abs * sign(r) + (2.0 * c_sq) * r) + c_grad * g;
}

// dL/dD and dL/dA of a valid pixel, each rounded once
S3Z_HD void grads(double dldr, float Df, float Af, double s, float& gd, float& ga) {
  const double D = (double)Df, A = (double)Af;
  gd = (float)(dldr * (s / A));
  ga = (float)(-(dldr * ((s * D) / (A * A))));
}

}  // namespace s3z
