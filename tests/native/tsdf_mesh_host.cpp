// Host build of csrc/tsdf_mesh_math.hpp (tests/test_tsdf_mesh.py): the
// arithmetic of s3f_integrate and s3f_mesh_count / s3f_mesh_emit on the CPU,
// voxel by voxel, as the kernels apply it.
//
//   tsdf_mesh_host integrate IN OUT nx ny nz V H W has_color has_wmap
// IN : {ox, oy, oz, voxel, trunc, w_max} f32, tsdf [n] f32, weight [n] f32,
//      rgb [3,n] f32, depth [V,H,W] f32, color [V,3,H,W] f32 (has_color),
//      wmap [V,H,W] f32 (has_wmap), K [V,9] f32, T_WC [V,16] f32
// OUT: tsdf, weight, rgb
//
//   tsdf_mesh_host mesh IN OUT nx ny nz
// IN : {ox, oy, oz, voxel, w_min} f32, tsdf [n], weight [n], rgb [3,n]
// OUT: {nv, nt} i64, verts [nv,3] f32, vcol [nv,3] f32, faces [nt,3] i32
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsdf_mesh_math.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}
template <class T>
static bool wr(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

static int run_integrate(char** a) {
  const long nx = atol(a[4]), ny = atol(a[5]), nz = atol(a[6]), V = atol(a[7]), H = atol(a[8]),
             W = atol(a[9]);
  const bool has_color = atol(a[10]) != 0, has_wmap = atol(a[11]) != 0;
  if (nx <= 0 || ny <= 0 || nz <= 0 || V <= 0 || H <= 0 || W <= 0) return 2;
  const long n = nx * ny * nz, plane = H * W;
  std::vector<float> par(6), tsdf(n), weight(n), rgb(3 * n), depth(V * plane),
      color(has_color ? V * 3 * plane : 0), wmap(has_wmap ? V * plane : 0), K(V * 9), T(V * 16);
  FILE* f = fopen(a[2], "rb");
  if (!f || !rd(f, par) || !rd(f, tsdf) || !rd(f, weight) || !rd(f, rgb) || !rd(f, depth) ||
      !rd(f, color) || !rd(f, wmap) || !rd(f, K) || !rd(f, T)) {
    fprintf(stderr, "short input\n");
    return 1;
  }
  fclose(f);
  std::vector<double> views(V * s3f::kView);
  for (long v = 0; v < V; ++v) {
    double vw[s3f::kView];
    s3f::prepare_view(&K[v * 9], &T[v * 16], vw);
    for (int j = 0; j < s3f::kView; ++j) views[v * s3f::kView + j] = vw[j];
  }
  for (long p = 0; p < n; ++p) {
    const int i = (int)(p % nx), j = (int)((p / nx) % ny), k = (int)(p / (nx * ny));
    double xw[3];
    s3f::voxel_centre(par[0], par[1], par[2], par[3], i, j, k, xw);
    float fv = tsdf[p], w = weight[p], c[3] = {rgb[p], rgb[n + p], rgb[2 * n + p]};
    bool any = false;
    for (long v = 0; v < V; ++v)
      any |= s3f::integrate_view(&views[v * s3f::kView], xw, (int)H, (int)W, &depth[v * plane],
                                 has_color ? &color[v * 3 * plane] : nullptr,
                                 has_wmap ? &wmap[v * plane] : nullptr, par[4], par[5], fv, w, c);
    if (!any) continue;
    tsdf[p] = fv;
    weight[p] = w;
    if (has_color)
      for (int ch = 0; ch < 3; ++ch) rgb[ch * n + p] = c[ch];
  }
  f = fopen(a[3], "wb");
  if (!f || !wr(f, tsdf) || !wr(f, weight) || !wr(f, rgb)) return 1;
  fclose(f);
  return 0;
}

static int run_mesh(char** a) {
  const long nx = atol(a[4]), ny = atol(a[5]), nz = atol(a[6]);
  if (nx <= 0 || ny <= 0 || nz <= 0) return 2;
  const long n = nx * ny * nz, nxny = nx * ny;
  std::vector<float> par(5), tsdf(n), weight(n), rgb(3 * n);
  FILE* f = fopen(a[2], "rb");
  if (!f || !rd(f, par) || !rd(f, tsdf) || !rd(f, weight) || !rd(f, rgb)) {
    fprintf(stderr, "short input\n");
    return 1;
  }
  fclose(f);
  const float w_min = par[4];
  auto corner = [&](long p, int c) { return p + (c & 1) + nx * ((c >> 1) & 1) + nxny * ((c >> 2) & 1); };
  auto inside_of = [&](long p) {
    unsigned m = 0;
    for (int c = 0; c < 8; ++c) m |= (tsdf[corner(p, c)] < 0.0f ? 1u : 0u) << c;
    return m;
  };
  const long dim[3] = {nx, ny, nz}, stride[3] = {1, nx, nxny};
  std::vector<unsigned char> cell_tris(n, 0), vert_mask(n, 0);
  for (long p = 0; p < n; ++p) {
    const long i = p % nx, j = (p / nx) % ny, k = p / nxny;
    if (!(i < nx - 1 && j < ny - 1 && k < nz - 1)) continue;
    bool valid = true;
    for (int c = 0; c < 8; ++c) valid = valid && weight[corner(p, c)] >= w_min;
    if (valid) cell_tris[p] = (unsigned char)s3f::cell_triangles(inside_of(p));
  }
  std::vector<int64_t> vbase(n, 0), tbase(n, 0);
  int64_t nv = 0, nt = 0;
  for (long p = 0; p < n; ++p) {
    const long x[3] = {p % nx, (p / nx) % ny, p / nxny};
    const bool in_p = tsdf[p] < 0.0f;
    unsigned mask = 0;
    for (int d = 0; d < 7; ++d) {
      const int code = s3f::dir_code(d);
      bool ok = true;
      for (int ax = 0; ax < 3; ++ax)
        if ((code >> ax) & 1) ok = ok && x[ax] + 1 < dim[ax];
      if (!ok || (tsdf[corner(p, code)] < 0.0f) == in_p) continue;
      bool live = false;
      for (int o = 0; o < 8; ++o) {
        if (o & code) continue;
        bool in_range = true;
        long cell = p;
        for (int ax = 0; ax < 3; ++ax) {
          const long ca = x[ax] - ((o >> ax) & 1);
          in_range = in_range && ca >= 0 && ca < dim[ax] - 1;
          cell -= stride[ax] * ((o >> ax) & 1);
        }
        if (in_range && cell_tris[cell] != 0) live = true;
      }
      if (live) mask |= 1u << d;
    }
    vert_mask[p] = (unsigned char)mask;
    vbase[p] = nv;
    nv += __builtin_popcount(mask);
    tbase[p] = nt;
    nt += cell_tris[p];
  }
  std::vector<float> verts(nv * 3), vcol(nv * 3);
  std::vector<int32_t> faces(nt * 3);
  for (long p = 0; p < n; ++p) {
    int64_t idx = vbase[p];
    for (int d = 0; d < 7; ++d) {
      if (!((vert_mask[p] >> d) & 1)) continue;
      const long q = corner(p, s3f::dir_code(d));
      const float ca[3] = {rgb[p], rgb[n + p], rgb[2 * n + p]};
      const float cb[3] = {rgb[q], rgb[n + q], rgb[2 * n + q]};
      float pos[3], col[3];
      s3f::edge_vertex(par[0], par[1], par[2], par[3], (int)(p % nx), (int)((p / nx) % ny),
                       (int)(p / nxny), d, tsdf[p], tsdf[q], ca, cb, pos, col);
      for (int ax = 0; ax < 3; ++ax) {
        verts[idx * 3 + ax] = pos[ax];
        vcol[idx * 3 + ax] = col[ax];
      }
      ++idx;
    }
  }
  for (long p = 0; p < n; ++p) {
    if (!cell_tris[p]) continue;
    const unsigned inside = inside_of(p);
    int64_t idx = tbase[p];
    for (int t = 0; t < 6; ++t) {
      int64_t tri[2][3];
      const int m = s3f::tet_triangles(t, inside, p, nx, nxny, tri);
      for (int s = 0; s < m; ++s, ++idx)
        for (int ax = 0; ax < 3; ++ax) {
          const int64_t owner = tri[s][ax] / 7;
          const int d = (int)(tri[s][ax] % 7);
          faces[idx * 3 + ax] =
              (int32_t)(vbase[owner] + __builtin_popcount(vert_mask[owner] & ((1u << d) - 1u)));
        }
    }
  }
  std::vector<int64_t> counts = {nv, nt};
  f = fopen(a[3], "wb");
  if (!f || !wr(f, counts) || !wr(f, verts) || !wr(f, vcol) || !wr(f, faces)) return 1;
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 12 && !strcmp(argv[1], "integrate")) return run_integrate(argv);
  if (argc == 7 && !strcmp(argv[1], "mesh")) return run_mesh(argv);
  fprintf(stderr,
          "usage: %s integrate IN OUT nx ny nz V H W has_color has_wmap\n"
          "       %s mesh IN OUT nx ny nz\n", argv[0], argv[0]);
  return 2;
}
