// Host restatement of the grid nearest-neighbour search and the mesh sampler:
// runs nn_search_math.hpp's s3k::cell_of / search / checked_area / face_weight
// / sample_* / pick_face / place, the functions the kernels of nn_search.hip
// call, on the CPU (tests/test_nn_search.py).  The grid build (count, exclusive
// sums, fill) and the cumulative weights are written out serially here.  Host
// code built with -ffp-contract=off.
//
//   nn_search_host nn IN OUT N M OX OY OZ CELL NX NY NZ MAX_DIST
//     IN:  ref [N, 3] float32, q [M, 3] float32
//     OUT: idx [M] int32, dist [M] float32, dropped int64, then per query
//          cells int64, rows int64 (what it visited), rings int32, linear int32
//   nn_search_host sample IN OUT V F S SEED
//     IN:  verts [V, 3] float32, faces [F, 3] int32
//     OUT: bad int64, total uint64, points [S, 3] float32, face [S] int32
//          (the last two absent when total = 0)
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

static int run_nn(char** a) {
  const int64_t n = atoll(a[2]), m = atoll(a[3]);
  s3k::Grid g{nullptr, nullptr, strtod(a[4], nullptr), strtod(a[5], nullptr),
              strtod(a[6], nullptr), strtod(a[7], nullptr), atoi(a[8]), atoi(a[9]), atoi(a[10])};
  const double max_dist = strtod(a[11], nullptr);
  const std::vector<char> in = read_all(a[0]);
  if (n < 0 || m < 0 || in.size() != (size_t)(n + m) * 12) {
    fprintf(stderr, "nn: %zu input bytes for n = %" PRId64 ", m = %" PRId64 "\n", in.size(), n, m);
    return 2;
  }
  const int64_t cells = s3k::cells_of(g);
  if (g.nx < 1 || g.ny < 1 || g.nz < 1 || cells > (1 << 27) || !(g.cell > 0.0)) {
    fprintf(stderr, "nn: bad grid\n");
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
    const float *r = &ref[3 * i];
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
  std::vector<int32_t> idx((size_t)m), rings((size_t)m), linear((size_t)m);
  std::vector<float> dist((size_t)m);
  std::vector<int64_t> vc((size_t)m), vr((size_t)m);
  for (int64_t j = 0; j < m; ++j) {
    s3k::Cost c;
    const s3k::Hit h = s3k::search(g, q[3 * j], q[3 * j + 1], q[3 * j + 2], max_dist, &c);
    idx[j] = h.i;
    dist[j] = (float)sqrt(h.d2);
    vc[j] = c.cells;
    vr[j] = c.rows;
    rings[j] = c.rings;
    linear[j] = c.linear ? 1 : 0;
  }
  std::vector<char> out;
  put(out, idx.data(), idx.size());
  put(out, dist.data(), dist.size());
  put(out, &dropped, 1);
  put(out, vc.data(), vc.size());
  put(out, vr.data(), vr.size());
  put(out, rings.data(), rings.size());
  put(out, linear.data(), linear.size());
  write_all(a[1], out);
  return 0;
}

static int run_sample(char** a) {
  const int64_t V = atoll(a[2]), F = atoll(a[3]), S = atoll(a[4]);
  const uint64_t seed = strtoull(a[5], nullptr, 0);
  const std::vector<char> in = read_all(a[0]);
  if (V < 0 || F < 0 || S < 0 || in.size() != (size_t)(V + F) * 12) {
    fprintf(stderr, "sample: %zu input bytes for V = %" PRId64 ", F = %" PRId64 "\n", in.size(), V,
            F);
    return 2;
  }
  std::vector<float> verts((size_t)V * 3 + 1);
  std::vector<int32_t> faces((size_t)F * 3 + 1);
  memcpy(verts.data(), in.data(), (size_t)V * 12);
  memcpy(faces.data(), in.data() + (size_t)V * 12, (size_t)F * 12);
  std::vector<double> area((size_t)F);
  int64_t n_bad = 0;
  double a_max = 0.0;
  for (int64_t f = 0; f < F; ++f) {
    bool bad;
    area[f] = s3k::checked_area(verts.data(), V, faces.data(), f, &bad);
    n_bad += bad ? 1 : 0;
    if (area[f] > a_max) a_max = area[f];
  }
  std::vector<uint64_t> C((size_t)F);
  uint64_t run = 0;
  for (int64_t f = 0; f < F; ++f) {
    run += s3k::face_weight(area[f], a_max);
    C[f] = run;
  }
  const uint64_t Q = run;
  std::vector<char> out;
  put(out, &n_bad, 1);
  put(out, &Q, 1);
  if (Q > 0) {
    std::vector<float> points((size_t)S * 3);
    std::vector<int32_t> face((size_t)S);
    for (int64_t k = 0; k < S; ++k) {
      double u[4];
      s3k::sample_uniforms(k, seed, u);
      const int64_t f = s3k::pick_face(C.data(), F, s3k::sample_target(k, u[0], S, Q));
      float p[3];
      s3k::place(&verts[3 * faces[3 * f]], &verts[3 * faces[3 * f + 1]],
                 &verts[3 * faces[3 * f + 2]], u[1], u[2], p);
      memcpy(&points[3 * k], p, sizeof(p));
      face[k] = (int32_t)f;
    }
    put(out, points.data(), points.size());
    put(out, face.data(), face.size());
  }
  write_all(a[1], out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 14 && !strcmp(argv[1], "nn")) return run_nn(argv + 2);
  if (argc == 8 && !strcmp(argv[1], "sample")) return run_sample(argv + 2);
  fprintf(stderr, "usage: see the head of tests/native/nn_search_host.cpp\n");
  return 2;
}
