// Host restatement of the pose gradient and pose step: runs
// pose_grad_math.hpp's functions, the ones the kernels of pose_grad.hip call,
// on the CPU (tests/test_pose_grad.py test_host_*).  Host code built with
// -ffp-contract=off.
//
//   pose_grad_host grad IN OUT MODE N RADII
//     MODE cov | rot; IN: float32 viewmatrix [16], means3D [N,3], d_means3D
//     [N,3], shape [N,k], d_shape [N,k] (k = 6 | 4), then int32 radii [N] when
//     RADII is 1.  OUT: float64 grad [6], then the skipped count as a float64.
//     The rows are summed in index order.
//   pose_grad_host step IN OUT STEPS
//     IN: float64 T [16], lr_translation, lr_rotation, beta1, beta2, eps,
//     render_scale, proj_t [16] (float32 values), then STEPS gradients [6].
//     OUT per step, float64: T [16], exp_avg [6], exp_avg_sq [6], then the
//     float32 camera widened: viewmatrix [16], projmatrix [16], campos [3].
//     The bias corrections are computed here, as the library's callers do.
//   pose_grad_host exp IN OUT
//     IN: float64 twists [k, 6]; OUT: float64 [k, 12], R [9] then V rho [3].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_grad_math.hpp"

static std::vector<char> read_all(const char* path) {
  std::vector<char> v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  char buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

static int write_all(const char* path, const std::vector<double>& out) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 2; }
  fwrite(out.data(), sizeof(double), out.size(), f);
  fclose(f);
  return 0;
}

static int run_grad(int argc, char** argv) {
  if (argc < 7) return 2;
  const bool cov = strcmp(argv[4], "cov") == 0;
  const size_t n = (size_t)atoll(argv[5]);
  const bool has_radii = atoi(argv[6]) == 1;
  const size_t k = cov ? 6 : 4;
  const std::vector<char> in = read_all(argv[2]);
  const size_t floats = 16 + n * (6 + 2 * k);
  if (in.size() != floats * 4 + (has_radii ? n * 4 : 0)) return 3;
  const float* f = reinterpret_cast<const float*>(in.data());
  const float *vm = f, *mu = f + 16, *dmu = mu + 3 * n, *sh = dmu + 3 * n, *dsh = sh + k * n;
  const int32_t* radii = has_radii ? reinterpret_cast<const int32_t*>(f + floats) : nullptr;
  s3x::Cam cam;
  s3x::cam_from_view(vm, cam);
  double acc[6] = {0, 0, 0, 0, 0, 0};
  double skipped = 0;
  for (size_t i = 0; i < n; ++i) {
    if (radii && radii[i] <= 0) continue;
    const float m3[3] = {mu[3 * i], mu[3 * i + 1], mu[3 * i + 2]};
    const float d3[3] = {dmu[3 * i], dmu[3 * i + 1], dmu[3 * i + 2]};
    bool ok;
    if (cov) {
      float c[6], d[6];
      memcpy(c, sh + 6 * i, sizeof(c));
      memcpy(d, dsh + 6 * i, sizeof(d));
      ok = s3x::sub_row_cov(cam, m3, d3, c, d, acc);
    } else {
      float q[4], d[4];
      memcpy(q, sh + 4 * i, sizeof(q));
      memcpy(d, dsh + 4 * i, sizeof(d));
      ok = s3x::sub_row_rot(cam, m3, d3, q, d, acc);
    }
    if (!ok) skipped += 1;
  }
  std::vector<double> out(acc, acc + 6);
  out.push_back(skipped);
  return write_all(argv[3], out);
}

static int run_step(int argc, char** argv) {
  if (argc < 5) return 2;
  const int steps = atoi(argv[4]);
  const std::vector<char> in = read_all(argv[2]);
  if (steps < 0 || in.size() != (size_t)(16 + 6 + 16 + 6 * steps) * 8) return 3;
  const double* d = reinterpret_cast<const double*>(in.data());
  double T[16], m[6] = {0, 0, 0, 0, 0, 0}, v[6] = {0, 0, 0, 0, 0, 0};
  memcpy(T, d, sizeof(T));
  s3x::PoseAdam hp{d[16], d[17], d[18], d[19], d[20], 1.0, 1.0, d[21]};
  float proj[16];
  for (int k = 0; k < 16; ++k) proj[k] = (float)d[22 + k];
  std::vector<double> out;
  for (int t = 1; t <= steps; ++t) {
    hp.bias1 = 1.0 - pow(hp.beta1, t);
    hp.bias2_sqrt = sqrt(1.0 - pow(hp.beta2, t));
    double g[6];
    memcpy(g, d + 38 + 6 * (t - 1), sizeof(g));
    s3x::pose_step(T, m, v, g, hp);
    float view[16], full[16], campos[3];
    s3x::pose_camera(T, hp.render_scale, proj, view, full, campos);
    out.insert(out.end(), T, T + 16);
    out.insert(out.end(), m, m + 6);
    out.insert(out.end(), v, v + 6);
    for (int k = 0; k < 16; ++k) out.push_back((double)view[k]);
    for (int k = 0; k < 16; ++k) out.push_back((double)full[k]);
    for (int k = 0; k < 3; ++k) out.push_back((double)campos[k]);
  }
  return write_all(argv[3], out);
}

static int run_exp(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::vector<char> in = read_all(argv[2]);
  if (in.size() % 48 != 0) return 3;
  const double* d = reinterpret_cast<const double*>(in.data());
  std::vector<double> out;
  for (size_t i = 0; i < in.size() / 48; ++i) {
    double xi[6], R[9], p[3];
    memcpy(xi, d + 6 * i, sizeof(xi));
    s3x::se3_exp(xi, R, p);
    out.insert(out.end(), R, R + 9);
    out.insert(out.end(), p, p + 3);
  }
  return write_all(argv[3], out);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (strcmp(argv[1], "grad") == 0) return run_grad(argc, argv);
  if (strcmp(argv[1], "step") == 0) return run_step(argc, argv);
  if (strcmp(argv[1], "exp") == 0) return run_exp(argc, argv);
  return 2;
}
