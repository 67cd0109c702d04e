// Host check of raster_math.hpp sh_basis / sh_basis_grad for deg 0..3
// (tests/test_raster_grad.py test_sh_basis_and_grad_native) on random unit
// vectors rounded to float:
//   sh_basis      against the real-SH closed forms in double, normalisation
//                 constants from their sqrt(./pi) expressions;
//   sh_basis_grad against central differences (h = 1e-4) of those closed
//                 forms in double, each coordinate independently (the kernel
//                 applies d normalize / d o separately).
//
// Bound.  With |x|, |y|, |z| <= 1 every entry is a constant times a
// polynomial of at most 7 float operations, plus the rounding of the
// constant: <= 8 roundings, each at most u = 2^-24 relative to a partial
// result no larger than M = |constant| * (sum of the polynomial's absolute
// monomial coefficients).  The largest M is 0.3732 * (2 + 3 + 3) < 3.0 for
// the basis (entry 12) and 0.3732 * (6 + 3 + 3) < 4.5 for the gradient
// (dZ of entry 12).  So
//   |basis - closed form| <= 8 u 3.0 = 1.44e-6
//   |grad  - difference | <= 8 u 4.5 + 1e-7 = 2.25e-6
// where 1e-7 covers the central difference itself: the entries are cubics,
// truncation h^2 / 6 * |f'''| <= 1e-8 / 6 * 20 = 3.4e-8, and double rounding
// 3 * 2.3e-16 / 1e-4 = 7e-12.
// Entries at and past (deg + 1)^2 must stay untouched (basis) / zero (grad).
// Prints "<vectors> <max basis err / bound> <max grad err / bound> <stray>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "raster_math.hpp"

static void closed_form(int deg, double x, double y, double z, double* B) {
  const double pi = 3.14159265358979323846;
  B[0] = 0.5 * std::sqrt(1.0 / pi);
  if (deg < 1) return;
  const double c1 = std::sqrt(3.0 / (4.0 * pi));
  B[1] = -c1 * y; B[2] = c1 * z; B[3] = -c1 * x;
  if (deg < 2) return;
  const double a2 = 0.5 * std::sqrt(15.0 / pi), b2 = 0.25 * std::sqrt(5.0 / pi);
  B[4] = a2 * x * y;
  B[5] = -a2 * y * z;
  B[6] = b2 * (2.0 * z * z - x * x - y * y);
  B[7] = -a2 * x * z;
  B[8] = 0.5 * a2 * (x * x - y * y);
  if (deg < 3) return;
  const double a3 = 0.25 * std::sqrt(35.0 / (2.0 * pi)), b3 = 0.5 * std::sqrt(105.0 / pi);
  const double c3 = 0.25 * std::sqrt(21.0 / (2.0 * pi)), d3 = 0.25 * std::sqrt(7.0 / pi);
  B[9] = -a3 * y * (3.0 * x * x - y * y);
  B[10] = b3 * x * y * z;
  B[11] = -c3 * y * (4.0 * z * z - x * x - y * y);
  B[12] = d3 * z * (2.0 * z * z - 3.0 * x * x - 3.0 * y * y);
  B[13] = -c3 * x * (4.0 * z * z - x * x - y * y);
  B[14] = 0.5 * b3 * z * (x * x - y * y);
  B[15] = -a3 * x * (x * x - 3.0 * y * y);
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 20000;
  const double u = std::ldexp(1.0, -24);
  const double bound_b = 8.0 * u * 3.0, bound_g = 8.0 * u * 4.5 + 1e-7, h = 1e-4;
  std::mt19937 rng(4321);
  std::normal_distribution<double> N(0.0, 1.0);
  double worst_b = 0.0, worst_g = 0.0;
  long stray = 0;
  for (int it = 0; it < n; ++it) {
    double v[3] = {N(rng), N(rng), N(rng)};
    const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (len < 1e-3) { --it; continue; }
    const float x = (float)(v[0] / len), y = (float)(v[1] / len), z = (float)(v[2] / len);
    for (int deg = 0; deg <= 3; ++deg) {
      const int nb = (deg + 1) * (deg + 1);
      float B[16], dX[16], dY[16], dZ[16];
      for (int k = 0; k < 16; ++k) B[k] = -77.0f;
      gsr::sh_basis(deg, x, y, z, B);
      gsr::sh_basis_grad(deg, x, y, z, dX, dY, dZ);
      double R[16], Rp[16], Rm[16];
      closed_form(deg, x, y, z, R);
      for (int k = 0; k < 16; ++k) {
        if (k < nb) continue;
        if (B[k] != -77.0f || dX[k] != 0.0f || dY[k] != 0.0f || dZ[k] != 0.0f) ++stray;
      }
      for (int k = 0; k < nb; ++k) worst_b = std::fmax(worst_b, std::fabs(B[k] - R[k]) / bound_b);
      const float* got[3] = {dX, dY, dZ};
      for (int ax = 0; ax < 3; ++ax) {
        double p[3] = {x, y, z}, m[3] = {x, y, z};
        p[ax] += h; m[ax] -= h;
        closed_form(deg, p[0], p[1], p[2], Rp);
        closed_form(deg, m[0], m[1], m[2], Rm);
        for (int k = 0; k < nb; ++k) {
          const double fd = (Rp[k] - Rm[k]) / (2.0 * h);
          worst_g = std::fmax(worst_g, std::fabs(got[ax][k] - fd) / bound_g);
        }
      }
    }
  }
  printf("%d %.6f %.6f %ld\n", n, worst_b, worst_g, stray);
  return 0;
}
