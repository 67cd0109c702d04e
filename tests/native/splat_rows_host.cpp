// Host restatement of the splat export / import arithmetic: runs
// splat_math.hpp's s3w::splat_row / s3w::splat_unpack, the functions the
// kernels of splat_io.hip call, on the CPU (tests/test_splat_io.py
// test_host_math_*).  Host code built by hipcc with -ffp-contract=off.
//
//   splat_rows_host export IN OUT SCALE_MIN   IN: [n, 13] float32 records
//       (mean 3, cov_triu 6, colour 3, opacity), OUT: [n, 17] rows
//   splat_rows_host import IN OUT             IN: [n, 14], OUT: [n, 13]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "splat_math.hpp"

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
  if (argc < 4) return 2;
  const bool exporting = strcmp(argv[1], "export") == 0;
  const std::vector<float> in = read_all(argv[2]);
  const int wi = exporting ? 13 : s3w::kRow14Floats, wo = exporting ? s3w::kRowFloats : 13;
  if (in.size() % wi != 0) return 3;
  const size_t n = in.size() / wi;
  std::vector<float> out(n * wo);
  if (exporting) {
    if (argc < 5) return 2;
    const float scale_min = (float)atof(argv[4]);
    for (size_t i = 0; i < n; ++i) {
      const float* r = &in[i * 13];
      const float mean[3] = {r[0], r[1], r[2]};
      const float cov[6] = {r[3], r[4], r[5], r[6], r[7], r[8]};
      const float col[3] = {r[9], r[10], r[11]};
      float row[s3w::kRowFloats];
      s3w::splat_row(mean, cov, col, r[12], scale_min, row);
      memcpy(&out[i * wo], row, sizeof(row));
    }
  } else {
    for (size_t i = 0; i < n; ++i) {
      float r[s3w::kRow14Floats], mean[3], cov[6], col[3], op;
      memcpy(r, &in[i * wi], sizeof(r));
      s3w::splat_unpack(r, mean, cov, col, op);
      float* o = &out[i * wo];
      memcpy(o, mean, 12);
      memcpy(o + 3, cov, 24);
      memcpy(o + 9, col, 12);
      o[12] = op;
    }
  }
  FILE* f = fopen(argv[3], "wb");
  if (!f) { perror(argv[3]); return 2; }
  fwrite(out.data(), sizeof(float), out.size(), f);
  fclose(f);
  return 0;
}
