// Host restatement of the splat optimiser's arithmetic: runs
// splat_opt_math.hpp's s3o::activate / s3o::adam_row, the functions the
// kernels of splat_opt.hip call, on the CPU (tests/test_refine.py
// test_host_math_*).  Host code built with -ffp-contract=off.
//
//   splat_opt_host IN OUT STEPS SCALE LR0 LR1 LR2 LR3 LR4 BETA1 BETA2 EPS
//   IN:  rows14 [n, 14], then STEPS blocks of gradients [n, 14]
//        (dmeans3D 3, dshs 3, dopacity 1, dscales 3, drotations 4), float32
//   OUT: the activations of the rows as given [n, 14] (same column groups),
//        then per step rows14, exp_avg, exp_avg_sq ([n, 14] each)
// The bias corrections are computed here in double, as the library's callers do.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "splat_opt_math.hpp"

static std::vector<float> read_all(const char* path) {
  std::vector<float> v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  float buf[4096];
  size_t k;
  while ((k = fread(buf, sizeof(float), 4096, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 13) return 2;
  constexpr int W = s3o::kRow;
  const std::vector<float> in = read_all(argv[1]);
  const int steps = atoi(argv[3]);
  const float s = (float)atof(argv[4]);
  float lr[s3o::kGroups];
  for (int k = 0; k < s3o::kGroups; ++k) lr[k] = (float)atof(argv[5 + k]);
  const float beta1 = (float)atof(argv[10]), beta2 = (float)atof(argv[11]);
  const float eps = (float)atof(argv[12]);
  if (steps < 0 || in.size() % ((size_t)W * (steps + 1)) != 0) return 3;
  const size_t n = in.size() / ((size_t)W * (steps + 1));
  std::vector<float> rows(in.begin(), in.begin() + n * W), m(n * W, 0.f), v(n * W, 0.f);
  std::vector<float> out;
  out.reserve(n * W * (1 + 3 * steps));
  for (size_t i = 0; i < n; ++i) {
    float r[W], a[W];
    memcpy(r, &rows[i * W], sizeof(r));
    float mean[3], sh[3], sc[3], q[4];
    s3o::activate(r, s, mean, sh, a[6], sc, q);
    memcpy(a, mean, sizeof(mean));
    memcpy(a + 3, sh, sizeof(sh));
    memcpy(a + 7, sc, sizeof(sc));
    memcpy(a + 10, q, sizeof(q));
    out.insert(out.end(), a, a + W);
  }
  for (int t = 1; t <= steps; ++t) {
    const float bias1 = (float)(1.0 - pow((double)beta1, t));
    const float bias2_sqrt = (float)sqrt(1.0 - pow((double)beta2, t));
    const float* G = &in[(size_t)t * n * W];
    for (size_t i = 0; i < n; ++i) {
      float r[W], mm[W], vv[W];
      memcpy(r, &rows[i * W], sizeof(r));
      memcpy(mm, &m[i * W], sizeof(mm));
      memcpy(vv, &v[i * W], sizeof(vv));
      const float* g = G + i * W;
      const float dmean[3] = {g[0], g[1], g[2]}, dsh[3] = {g[3], g[4], g[5]};
      const float dsc[3] = {g[7], g[8], g[9]}, dq[4] = {g[10], g[11], g[12], g[13]};
      if (s3o::all_finite(dmean, dsh, g[6], dsc, dq))
        s3o::adam_row(r, mm, vv, s, dmean, dsh, g[6], dsc, dq, lr, beta1, beta2, eps, bias1,
                      bias2_sqrt);
      memcpy(&rows[i * W], r, sizeof(r));
      memcpy(&m[i * W], mm, sizeof(mm));
      memcpy(&v[i * W], vv, sizeof(vv));
    }
    out.insert(out.end(), rows.begin(), rows.end());
    out.insert(out.end(), m.begin(), m.end());
    out.insert(out.end(), v.begin(), v.end());
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  fwrite(out.data(), sizeof(float), out.size(), f);
  fclose(f);
  return 0;
}
