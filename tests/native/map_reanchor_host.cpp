// Host build of csrc/map_reanchor_math.hpp (tests/test_map_reanchor.py): the
// arithmetic of s3a_map_reanchor on the CPU, row by row, as the two kernels
// apply it.
//
//   map_reanchor_host IN OUT n cap n_kf
// IN : means [cap,3] f32, cov_triu [cap,6] f32, kf_id [cap] i32,
//      anchor [n_kf,8] f32, poses [n_kf,8] f32
// OUT: means, cov_triu, anchor (as above), moved i64, held i64
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "map_reanchor_math.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v) {
  return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}
template <class T>
static bool wr(FILE* f, const std::vector<T>& v) {
  return fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s IN OUT n cap n_kf\n", argv[0]);
    return 2;
  }
  const long n = atol(argv[3]), cap = atol(argv[4]), n_kf = atol(argv[5]);
  if (n < 0 || cap < n || n_kf <= 0) return 2;
  std::vector<float> means(cap * 3), cov(cap * 6), anchor(n_kf * 8), poses(n_kf * 8);
  std::vector<int32_t> kf(cap);
  FILE* f = fopen(argv[1], "rb");
  if (!f || !rd(f, means) || !rd(f, cov) || !rd(f, kf) || !rd(f, anchor) || !rd(f, poses)) {
    fprintf(stderr, "short input\n");
    return 1;
  }
  fclose(f);
  std::vector<double> delta(n_kf * s3a::kDelta);
  std::vector<int64_t> tally(2, 0);
  for (long k = 0; k < n_kf; ++k) {
    double d[s3a::kDelta];
    bool adopt;
    if (s3a::classify(&anchor[k * 8], &poses[k * 8], d, adopt)) ++tally[1];
    for (int j = 0; j < s3a::kDelta; ++j) delta[k * s3a::kDelta + j] = d[j];
    if (adopt)
      for (int j = 0; j < 8; ++j) anchor[k * 8 + j] = poses[k * 8 + j];
  }
  for (long i = 0; i < n; ++i) {
    const int32_t k = kf[i];
    if (k < 0 || k >= n_kf || delta[(long)k * s3a::kDelta] == 0.0) continue;
    float mu[3] = {means[i * 3], means[i * 3 + 1], means[i * 3 + 2]};
    float c6[6];
    for (int j = 0; j < 6; ++j) c6[j] = cov[i * 6 + j];
    s3a::move_row(&delta[(long)k * s3a::kDelta], mu, c6);
    for (int j = 0; j < 3; ++j) means[i * 3 + j] = mu[j];
    for (int j = 0; j < 6; ++j) cov[i * 6 + j] = c6[j];
    ++tally[0];
  }
  f = fopen(argv[2], "wb");
  if (!f || !wr(f, means) || !wr(f, cov) || !wr(f, anchor) || !wr(f, tally)) return 1;
  fclose(f);
  return 0;
}
