// Host restatement of the k-nearest search: runs nn_search_math.hpp's
// s3k::search_k / emit_k, the functions k_nn_knn of nn_search.hip calls, on
// the CPU (tests/test_knn.py), with the slot capacity chosen as s3k_knn
// chooses it.  The grid build (count, exclusive sums, fill) is written out
// serially here.  Host code built with -ffp-contract=off.
//
//   knn_host IN OUT N M OX OY OZ CELL NX NY NZ MAX_DIST K EXCLUDE_SELF
//     IN:  ref [N, 3] float32, q [M, 3] float32
//     OUT: idx [M, K] int32, dist [M, K] float32, mean_d [M] float32,
//          mean_d2 [M] float32, then per query cells int64, rows int64 (what it
//          visited), rings int32, linear int32
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nn_search_math.hpp"

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

template <typename T>
static void put(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); }
}

template <int CAP>
static s3k::RowStats one(const s3k::Grid& g, const float* q, int32_t k, int32_t self,
                         double max_dist, int32_t* idx, float* dist, s3k::Cost* c) {
  s3k::HitK<CAP> h;
  s3k::search_k(g, q[0], q[1], q[2], k, self, max_dist, h, c);
  return s3k::emit_k(h, k, idx, dist);
}

int main(int argc, char** argv) {
  if (argc != 15) {
    fprintf(stderr, "usage: see the head of tests/native/knn_host.cpp\n");
    return 2;
  }
  char** a = argv + 1;
  const int64_t n = atoll(a[2]), m = atoll(a[3]);
  s3k::Grid g{nullptr, nullptr, strtod(a[4], nullptr), strtod(a[5], nullptr),
              strtod(a[6], nullptr), strtod(a[7], nullptr), atoi(a[8]), atoi(a[9]), atoi(a[10])};
  const double max_dist = strtod(a[11], nullptr);
  const int32_t k = atoi(a[12]);
  const bool exclude_self = atoi(a[13]) != 0;
  const std::vector<char> in = read_all(a[0]);
  if (n < 0 || m < 0 || in.size() != (size_t)(n + m) * 12) {
    fprintf(stderr, "knn: %zu input bytes for n = %" PRId64 ", m = %" PRId64 "\n", in.size(), n, m);
    return 2;
  }
  const int64_t cells = s3k::cells_of(g);
  if (g.nx < 1 || g.ny < 1 || g.nz < 1 || cells > (1 << 27) || !(g.cell > 0.0) || k < 1 ||
      k > 32 || (exclude_self && m > n)) {
    fprintf(stderr, "knn: bad arguments\n");
    return 2;
  }
  std::vector<float> ref((size_t)n * 3 + 1), q((size_t)m * 3 + 1);
  memcpy(ref.data(), in.data(), (size_t)n * 12);
  memcpy(q.data(), in.data() + (size_t)n * 12, (size_t)m * 12);
  // build: cell ids, counts, exclusive sums, fill
  std::vector<uint32_t> start((size_t)cells + 1, 0u), cursor((size_t)cells, 0u);
  std::vector<int64_t> cid((size_t)n, -1);
  int64_t dropped = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* r = &ref[3 * i];
    if (!s3k::finite3(r[0], r[1], r[2])) { ++dropped; continue; }
    cid[i] = s3k::cell_of(g, r[0], r[1], r[2]);
    ++start[cid[i] + 1];
  }
  for (int64_t c = 0; c < cells; ++c) start[c + 1] += start[c];
  std::vector<s3k::Rec> rec((size_t)(n - dropped) + 1);
  for (int64_t i = 0; i < n; ++i) {
    if (cid[i] < 0) continue;
    rec[start[cid[i]] + cursor[cid[i]]++] = s3k::Rec{ref[3 * i], ref[3 * i + 1], ref[3 * i + 2],
                                                     (int32_t)i};
  }
  g.start = start.data();
  g.rec = rec.data();
  std::vector<int32_t> idx((size_t)m * k), rings((size_t)m), linear((size_t)m);
  std::vector<float> dist((size_t)m * k), mean_d((size_t)m), mean_d2((size_t)m);
  std::vector<int64_t> vc((size_t)m), vr((size_t)m);
  for (int64_t j = 0; j < m; ++j) {
    s3k::Cost c;
    const int32_t self = exclude_self ? (int32_t)j : -1;
    int32_t* ip = &idx[(size_t)j * k];
    float* dp = &dist[(size_t)j * k];
    const float* qp = &q[3 * j];
    const s3k::RowStats o = k <= 4    ? one<4>(g, qp, k, self, max_dist, ip, dp, &c)
                            : k <= 8  ? one<8>(g, qp, k, self, max_dist, ip, dp, &c)
                            : k <= 16 ? one<16>(g, qp, k, self, max_dist, ip, dp, &c)
                                      : one<32>(g, qp, k, self, max_dist, ip, dp, &c);
    mean_d[j] = o.mean_d;
    mean_d2[j] = o.mean_d2;
    vc[j] = c.cells;
    vr[j] = c.rows;
    rings[j] = c.rings;
    linear[j] = c.linear ? 1 : 0;
  }
  FILE* f = fopen(a[1], "wb");
  if (!f) { perror(a[1]); return 2; }
  put(f, idx);
  put(f, dist);
  put(f, mean_d);
  put(f, mean_d2);
  put(f, vc);
  put(f, vr);
  put(f, rings);
  put(f, linear);
  fclose(f);
  return 0;
}
