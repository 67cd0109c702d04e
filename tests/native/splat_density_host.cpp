// Host restatement of adaptive density control: runs splat_density_math.hpp's
// s3d::philox4x32_10 / decide / split_child / grad_norm2d, the functions the
// kernels of splat_density.hip call, on the CPU (tests/test_density.py).  The
// capacity rule and the output order of include/s3d.h are written out
// sequentially here.  Host code built with -ffp-contract=off.
//
//   splat_density_host philox C0 C1 C2 C3 K0 K1            (hex words)
//     prints the four output words in hex
//   splat_density_host densify IN OUT N CAP GRAD_THRESHOLD SPLIT_SCALE
//                      MIN_OPACITY MAX_SCALE MAX_SCREEN_RADIUS SEED PASS
//     IN:  rows14, exp_avg, exp_avg_sq [N, 14] float32, grad_accum [N]
//          float32, denom [N] int32, max_radii [N] int32
//     OUT: n_out int64, counts int32[4], origin [n_out] int32, then rows14,
//          exp_avg, exp_avg_sq [n_out, 14] float32
//   splat_density_host accumulate IN OUT N STEPS
//     IN:  per step d_means2D [N, 3] float32 and radii [N] int32
//     OUT: grad_accum [N] float32, denom [N] int32, max_radii [N] int32
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "splat_density_math.hpp"

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

static void write_all(const char* path, const std::vector<char>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); exit(2); }
  fwrite(v.data(), 1, v.size(), f);
  fclose(f);
}

template <typename T>
static void put(std::vector<char>& out, const T* p, size_t count) {
  const char* c = reinterpret_cast<const char*>(p);
  out.insert(out.end(), c, c + count * sizeof(T));
}

static int run_philox(char** a) {
  uint32_t c[4];
  for (int k = 0; k < 4; ++k) c[k] = (uint32_t)strtoul(a[k], nullptr, 16);
  s3d::philox4x32_10(c, (uint32_t)strtoul(a[4], nullptr, 16), (uint32_t)strtoul(a[5], nullptr, 16));
  printf("%08x %08x %08x %08x\n", c[0], c[1], c[2], c[3]);
  return 0;
}

static int run_densify(char** a) {
  constexpr int W = s3d::kRow;
  const std::vector<char> in = read_all(a[0]);
  const int64_t n = atoll(a[2]), cap = atoll(a[3]);
  const s3d::Params p = {(float)atof(a[4]), (float)atof(a[5]), (float)atof(a[6]),
                         (float)atof(a[7]), (int32_t)atol(a[8])};
  const uint64_t seed = strtoull(a[9], nullptr, 0);
  const uint32_t pass = (uint32_t)strtoul(a[10], nullptr, 0);
  if (n < 0 || cap < n || in.size() != (size_t)n * (3 * W + 3) * 4) return 3;
  const float* rows = reinterpret_cast<const float*>(in.data());
  const float *m = rows + n * W, *v = m + n * W, *ga = v + n * W;
  const int32_t* dn = reinterpret_cast<const int32_t*>(ga + n);
  const int32_t* mr = dn + n;
  std::vector<int> code(n);
  int64_t B = 0, G = 0;
  for (int64_t i = 0; i < n; ++i) {
    float r[W];
    memcpy(r, rows + i * W, sizeof(r));
    code[i] = s3d::decide(r, ga[i], dn[i], mr[i], p);
    B += code[i] != s3d::kPrune;
    G += code[i] >= s3d::kClone;
  }
  const int64_t budget = cap - B;
  std::vector<float> orow, om, ov;
  std::vector<int32_t> origin;
  int32_t counts[4] = {(int32_t)(n - B), 0, 0, 0};
  const float zero[W] = {};
  int64_t grow_before = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (code[i] == s3d::kPrune) continue;
    const bool asks = code[i] >= s3d::kClone;
    const bool grows = asks && grow_before < budget;
    if (asks) ++grow_before;
    if (asks && !grows) ++counts[3];
    float r[W];
    memcpy(r, rows + i * W, sizeof(r));
    if (grows && code[i] == s3d::kSplit) {
      for (uint32_t k = 0; k < 2; ++k) {
        float c[W];
        s3d::split_child(r, i, pass, k, seed, c);
        orow.insert(orow.end(), c, c + W);
        om.insert(om.end(), zero, zero + W);
        ov.insert(ov.end(), zero, zero + W);
        origin.push_back(~(int32_t)i);
      }
      ++counts[2];
      continue;
    }
    orow.insert(orow.end(), r, r + W);
    om.insert(om.end(), m + i * W, m + (i + 1) * W);
    ov.insert(ov.end(), v + i * W, v + (i + 1) * W);
    origin.push_back((int32_t)i);
    if (grows) {
      orow.insert(orow.end(), r, r + W);
      om.insert(om.end(), zero, zero + W);
      ov.insert(ov.end(), zero, zero + W);
      origin.push_back(~(int32_t)i);
      ++counts[1];
    }
  }
  const int64_t n_out = (int64_t)origin.size();
  std::vector<char> out;
  put(out, &n_out, 1);
  put(out, counts, 4);
  put(out, origin.data(), origin.size());
  put(out, orow.data(), orow.size());
  put(out, om.data(), om.size());
  put(out, ov.data(), ov.size());
  write_all(a[1], out);
  return 0;
}

static int run_accumulate(char** a) {
  const std::vector<char> in = read_all(a[0]);
  const int64_t n = atoll(a[2]);
  const int steps = atoi(a[3]);
  if (n < 0 || steps < 0 || in.size() != (size_t)n * 16 * steps) return 3;
  std::vector<float> ga(n, 0.f);
  std::vector<int32_t> dn(n, 0), mr(n, 0);
  for (int t = 0; t < steps; ++t) {
    const float* d2 = reinterpret_cast<const float*>(in.data() + (size_t)t * n * 16);
    const int32_t* radii = reinterpret_cast<const int32_t*>(d2 + n * 3);
    for (int64_t i = 0; i < n; ++i) {
      if (radii[i] <= 0) continue;
      const float g = s3d::grad_norm2d(d2[i * 3], d2[i * 3 + 1]);
      if (!(g >= 0.0f)) continue;
      ga[i] += g;
      dn[i] += 1;
      mr[i] = radii[i] > mr[i] ? radii[i] : mr[i];
    }
  }
  std::vector<char> out;
  put(out, ga.data(), ga.size());
  put(out, dn.data(), dn.size());
  put(out, mr.data(), mr.size());
  write_all(a[1], out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 8 && !strcmp(argv[1], "philox")) return run_philox(argv + 2);
  if (argc >= 13 && !strcmp(argv[1], "densify")) return run_densify(argv + 2);
  if (argc >= 6 && !strcmp(argv[1], "accumulate")) return run_accumulate(argv + 2);
  return 2;
}
