// Per-view, per-voxel and per-tetrahedron arithmetic of TSDF fusion and mesh
// extraction (tsdf_mesh.hip, include/s3f.h), host + device so a host program
// can restate it (tests/native/tsdf_mesh_host.cpp).
//
// Everything is double on the float32 inputs; the state of a voxel and the
// attributes of a vertex are rounded to float32 once.  Build with
// -ffp-contract=off: every product and sum rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define S3F_HD __host__ __device__ __forceinline__

namespace s3f {

// A prepared view: flag, B = M^T / s^2 (row-major), t, s, fx, fy, cx, cy.
constexpr int kView = 20;
enum : int { vFlag = 0, vB = 1, vT = 10, vS = 13, vFx = 14, vFy = 15, vCx = 16, vCy = 17 };

S3F_HD bool finite32(float v) { return fabsf(v) <= 3.402823466e+38f; }
S3F_HD bool finite64(double v) { return fabs(v) <= 1.7976931348623157e+308; }

// K [9] and T_WC [16] (row-major float32) -> the view record.  An invalid view
// gets flag 0 and is skipped by every voxel.
S3F_HD void prepare_view(const float* K, const float* T, double (&vw)[kView]) {
#pragma unroll
  for (int j = 0; j < kView; ++j) vw[j] = 0.0;
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  bool ok = finite32(fx) && finite32(fy) && finite32(cx) && finite32(cy) && fx > 0.0f && fy > 0.0f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) ok = ok && finite32(T[r * 4 + c]);
  if (!ok) return;
  const double m00 = T[0], m10 = T[4], m20 = T[8];
  const double s2 = m00 * m00 + m10 * m10 + m20 * m20;
  const double s = sqrt(s2);
  if (!(s > 0.0) || !finite64(s)) return;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) vw[vB + r * 3 + c] = (double)T[c * 4 + r] / s2;
#pragma unroll
  for (int r = 0; r < 3; ++r) vw[vT + r] = (double)T[r * 4 + 3];
  vw[vS] = s;
  vw[vFx] = fx;
  vw[vFy] = fy;
  vw[vCx] = cx;
  vw[vCy] = cy;
  vw[vFlag] = 1.0;
}

// The centre of voxel (i, j, k).
S3F_HD void voxel_centre(float ox, float oy, float oz, float voxel, int i, int j, int k,
                         double (&xw)[3]) {
  xw[0] = (double)ox + (double)voxel * (double)i;
  xw[1] = (double)oy + (double)voxel * (double)j;
  xw[2] = (double)oz + (double)voxel * (double)k;
}

// One view on one voxel (steps 1-9 of include/s3f.h).  depth, color and wmap
// are this view's planes (color, wmap may be null).  Returns whether the
// state (f, w, c[3]) was updated.
S3F_HD bool integrate_view(const double* vw, const double (&xw)[3], int H, int W,
                           const float* depth, const float* color, const float* wmap, float trunc,
                           float w_max, float& f, float& w, float (&c)[3]) {
  if (vw[vFlag] == 0.0) return false;
  const double e0 = xw[0] - vw[vT + 0], e1 = xw[1] - vw[vT + 1], e2 = xw[2] - vw[vT + 2];
  const double x = vw[vB + 0] * e0 + vw[vB + 1] * e1 + vw[vB + 2] * e2;
  const double y = vw[vB + 3] * e0 + vw[vB + 4] * e1 + vw[vB + 5] * e2;
  const double z = vw[vB + 6] * e0 + vw[vB + 7] * e1 + vw[vB + 8] * e2;
  if (!(z > 0.0)) return false;
  const double u = vw[vFx] * x / z + vw[vCx];
  const double v = vw[vFy] * y / z + vw[vCy];
  const double a = floor(u + 0.5), b = floor(v + 0.5);
  if (!(a >= 0.0 && a <= (double)(W - 1) && b >= 0.0 && b <= (double)(H - 1))) return false;
  const int64_t pix = (int64_t)b * W + (int64_t)a;
  const float d = depth[pix];
  if (!(finite32(d) && d > 0.0f)) return false;
  const float wo32 = wmap ? wmap[pix] : 1.0f;
  if (!(finite32(wo32) && wo32 > 0.0f)) return false;
  const double sdf = vw[vS] * ((double)d - z);
  if (sdf < -(double)trunc) return false;
  const double fo = fmin(1.0, sdf / (double)trunc);
  const double wv = w, wo = wo32, sum = wv + wo;
  f = (float)(((double)f * wv + fo * wo) / sum);
  if (color) {
    const int64_t plane = (int64_t)H * W;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      c[ch] = (float)(((double)c[ch] * wv + (double)color[ch * plane + pix] * wo) / sum);
  }
  w = (float)fmin(sum, (double)w_max);
  return true;
}

// ------------------------------------------------------ marching tetrahedra
// A cube corner is a 3-bit code dx + 2 dy + 4 dz.
// Direction d of the 7 edges a lattice point owns, as a corner code, and back.
S3F_HD int dir_code(int d) {
  constexpr int t[7] = {1, 2, 4, 3, 6, 5, 7};
  return t[d];
}
S3F_HD int code_dir(int code) {
  constexpr int t[8] = {-1, 0, 1, 3, 2, 5, 4, 6};
  return t[code];
}

// Corner codes of Kuhn tetrahedron t (permutations of the axes in
// lexicographic order): 0, e_a, e_a + e_b, 7.
S3F_HD void tet_corners(int t, int (&c)[4]) {
  constexpr int pa[6] = {0, 0, 1, 1, 2, 2};
  constexpr int pb[6] = {1, 2, 0, 2, 0, 1};
  c[0] = 0;
  c[1] = 1 << pa[t];
  c[2] = c[1] | (1 << pb[t]);
  c[3] = 7;
}

// Triangles of a cell whose corners' insideness is the 8-bit mask `inside`.
S3F_HD int cell_triangles(unsigned inside) {
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    int c[4];
    tet_corners(t, c);
    const int k = (int)((inside >> c[0]) & 1u) + (int)((inside >> c[1]) & 1u) +
                  (int)((inside >> c[2]) & 1u) + (int)((inside >> c[3]) & 1u);
    n += (k == 1 || k == 3) ? 1 : (k == 2 ? 2 : 0);
  }
  return n;
}

S3F_HD int det3(int a, int b, int c, int d) {
  // det(b - a, c - a, d - a) of four corner codes
  int v[3][3];
  const int q[3] = {b, c, d};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[r][k] = ((q[r] >> k) & 1) - ((a >> k) & 1);
  return v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) -
         v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
         v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
}

// Id of the edge between corners x and y (one a subset of the other) of the
// cell whose corner 000 is lattice point `cell` (linear index).
S3F_HD int64_t edge_id(int64_t cell, int64_t nx, int64_t nxny, int x, int y) {
  const int lo = x & y, hi = x | y;
  const int64_t p = cell + (lo & 1) + nx * ((lo >> 1) & 1) + nxny * ((lo >> 2) & 1);
  return 7 * p + code_dir(hi ^ lo);
}

// The triangles of tetrahedron t of a valid cell as edge ids, wound towards
// the outside corners.  Returns their number (0, 1 or 2).
S3F_HD int tet_triangles(int t, unsigned inside, int64_t cell, int64_t nx, int64_t nxny,
                         int64_t (&tri)[2][3]) {
  int c[4];
  tet_corners(t, c);
  int in[4], out[4], ni = 0, no = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if ((inside >> c[k]) & 1u)
      in[ni++] = c[k];
    else
      out[no++] = c[k];
  }
  if (ni == 0 || ni == 4) return 0;
  if (ni == 2) {
    const int a = in[0], b = in[1], cc = out[0], d = out[1];
    int64_t q[4] = {edge_id(cell, nx, nxny, a, cc), edge_id(cell, nx, nxny, a, d),
                    edge_id(cell, nx, nxny, b, d), edge_id(cell, nx, nxny, b, cc)};
    if (det3(a, b, cc, d) < 0) {
      int64_t s = q[0];
      q[0] = q[3];
      q[3] = s;
      s = q[1];
      q[1] = q[2];
      q[2] = s;
    }
    int m = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (q[k] < q[m]) m = k;
    tri[0][0] = q[m];
    tri[0][1] = q[(m + 1) & 3];
    tri[0][2] = q[(m + 2) & 3];
    tri[1][0] = q[m];
    tri[1][1] = q[(m + 2) & 3];
    tri[1][2] = q[(m + 3) & 3];
    return 2;
  }
  // one corner alone on its side: a, the others b, c, d in corner order
  const bool lone_in = ni == 1;
  const int a = lone_in ? in[0] : out[0];
  const int o[3] = {lone_in ? out[0] : in[0], lone_in ? out[1] : in[1], lone_in ? out[2] : in[2]};
  const bool away = det3(a, o[0], o[1], o[2]) > 0;   // (ab, ac, ad) has its normal away from a
  const bool flip = away != lone_in;                 // the normal leaves an inside a, faces an outside a
  tri[0][0] = edge_id(cell, nx, nxny, a, o[0]);
  tri[0][1] = edge_id(cell, nx, nxny, a, flip ? o[2] : o[1]);
  tri[0][2] = edge_id(cell, nx, nxny, a, flip ? o[1] : o[2]);
  return 1;
}

// Position and colour of the vertex on edge d of lattice point (i, j, k):
// fa, fb the tsdf at its ends, ca, cb their colours (null: no colour).
S3F_HD void edge_vertex(float ox, float oy, float oz, float voxel, int i, int j, int k, int d,
                        float fa, float fb, const float* ca, const float* cb, float (&pos)[3],
                        float (&col)[3]) {
  const double t = (double)fa / ((double)fa - (double)fb);
  const int code = dir_code(d);
  pos[0] = (float)((double)ox + (double)voxel * ((double)i + t * (double)(code & 1)));
  pos[1] = (float)((double)oy + (double)voxel * ((double)j + t * (double)((code >> 1) & 1)));
  pos[2] = (float)((double)oz + (double)voxel * ((double)k + t * (double)((code >> 2) & 1)));
  if (ca && cb) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      col[ch] = (float)((double)ca[ch] + t * ((double)cb[ch] - (double)ca[ch]));
  }
}

}  // namespace s3f
