// Arithmetic of the grid nearest-neighbour search and the mesh sampler
// (nn_search.hip, include/s3k.h), host + device so a host program can restate
// it (tests/native/nn_search_host.cpp).
//
// cell_axis()    cell of a coordinate, clamped as a double
// dist2()        squared distance in double, (dx dx + dy dy) + dz dz
// ring_done(), ring_past()   the two stop rules of the ring walk
// search()       one query: rings, then the linear rest when they stop paying
// HitK, insert_k(), search_k(), emit_k()   the same walk keeping the k nearest
//                rows in registers, and the row it writes
// face_area(), face_weight(), sample_uniforms(), sample_target(),
// pick_face(), place()       the sampler
// Build with -ffp-contract=off: every product and sum rounds once.
//
// Why the stop rule is conservative.  Let the query's (clamped) cell be c and
// a row's (clamped) cell be e with |e_a - c_a| = k > r on some axis a, say
// e_a > c_a.  Unclamped, floor((x - o) / cell) of the row is >= e_a (clamping
// from above only lowers it, and e_a > c_a >= 0 rules out clamping from
// below) and that of the query is <= c_a (likewise), so in exact arithmetic
// the coordinates differ by more than (k - 1) cell >= r cell.  The computed
// quotients carry a relative error of at most 3 x 2^-53 each, which the
// factor 1 - 2^-20 covers whenever |x - o| / cell < 2^32; beyond that the
// point is more than 2^32 - 2^27 cells outside the grid and k - 1 understates
// its distance by far more.  The comparison is strict, so a row at exactly
// the bound (a tie) is never given up either.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "splat_density_math.hpp"

#define S3K_HD __host__ __device__ __forceinline__

namespace s3k {

constexpr float kFltMax = 3.402823466e+38f;
constexpr double kMargin = 1.0 - 1.0 / 1048576.0;   // 1 - 2^-20
constexpr double kTwo32 = 4294967296.0;
constexpr int32_t kNoIndex = 0x7fffffff;

// one kept reference row, 16 bytes
struct Rec {
  float x, y, z;
  int32_t i;
};

struct Grid {
  const uint32_t* start;   // [cells + 1]
  const Rec* rec;          // [start[cells]]
  double ox, oy, oz, cell;
  int32_t nx, ny, nz;
};

struct Hit {
  double d2;
  int32_t i;               // -1: none
};

// what a query cost (the linear-rest rule reads it; the host program reports it)
struct Cost {
  int64_t cells, rows;
  int32_t rings;
  bool linear;
};

S3K_HD bool finite3(float x, float y, float z) {
  return fabsf(x) <= kFltMax && fabsf(y) <= kFltMax && fabsf(z) <= kFltMax;
}

S3K_HD int32_t cell_axis(float x, double origin, double cell, int32_t dim) {
  double t = floor(((double)x - origin) / cell);
  const double top = (double)(dim - 1);
  t = t < 0.0 ? 0.0 : (t > top ? top : t);
  return (int32_t)t;
}

S3K_HD int64_t cells_of(const Grid& g) { return (int64_t)g.nx * g.ny * g.nz; }

S3K_HD int32_t flat_cell(const Grid& g, int32_t cx, int32_t cy, int32_t cz) {
  return (cz * g.ny + cy) * g.nx + cx;
}

// cell id of a finite row
S3K_HD int32_t cell_of(const Grid& g, float x, float y, float z) {
  return flat_cell(g, cell_axis(x, g.ox, g.cell, g.nx), cell_axis(y, g.oy, g.cell, g.ny),
                   cell_axis(z, g.oz, g.cell, g.nz));
}

S3K_HD double dist2(double qx, double qy, double qz, float rx, float ry, float rz) {
  const double dx = qx - (double)rx, dy = qy - (double)ry, dz = qz - (double)rz;
  return (dx * dx + dy * dy) + dz * dz;
}

S3K_HD bool ring_done(double best_d2, int32_t r, double cell) {
  const double b = (double)r * cell * kMargin;
  return best_d2 < b * b;
}

S3K_HD bool ring_past(int32_t r, double cell, double max_dist) {
  return (double)r * cell * kMargin > max_dist;
}

// Who looks at the records of a run: Serial, one thread at all of them, or a
// set of lanes (nn_search.hip's WaveLanes) that take every step()-th record
// from first() and agree on the best of their hits in reduce().
struct Serial {
  S3K_HD uint32_t first() const { return 0u; }
  S3K_HD uint32_t step() const { return 1u; }
  S3K_HD void reduce(Hit&) const {}
};

// the records of cells id0 .. id1 (one contiguous run)
template <class L>
S3K_HD void scan_run(const Grid& g, int32_t id0, int32_t id1, double qx, double qy, double qz,
                     Hit& h, Cost& c, const L& lanes) {
  const uint32_t a = g.start[id0], b = g.start[id1 + 1];
  c.cells += id1 - id0 + 1;
  c.rows += b - a;
  for (uint32_t k = a + lanes.first(); k < b; k += lanes.step()) {
    const Rec r = g.rec[k];
    const double d2 = dist2(qx, qy, qz, r.x, r.y, r.z);
    if (d2 < h.d2 || (d2 == h.d2 && r.i < h.i)) {
      h.d2 = d2;
      h.i = r.i;
    }
  }
}

S3K_HD int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }
S3K_HD int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

// everything outside the cube [x0, x1] x [y0, y1] x [z0, z1] of cells
template <class L>
S3K_HD void scan_rest(const Grid& g, int32_t x0, int32_t x1, int32_t y0, int32_t y1, int32_t z0,
                      int32_t z1, double qx, double qy, double qz, Hit& h, Cost& c,
                      const L& lanes) {
  const int32_t slab = g.nx * g.ny;
  if (z0 > 0) scan_run(g, 0, z0 * slab - 1, qx, qy, qz, h, c, lanes);
  for (int32_t z = z0; z <= z1; ++z) {
    const int32_t zb = z * slab;
    if (y0 > 0) scan_run(g, zb, zb + y0 * g.nx - 1, qx, qy, qz, h, c, lanes);
    for (int32_t y = y0; y <= y1; ++y) {
      const int32_t b = zb + y * g.nx;
      if (x0 > 0) scan_run(g, b, b + x0 - 1, qx, qy, qz, h, c, lanes);
      if (x1 < g.nx - 1) scan_run(g, b + x1 + 1, b + g.nx - 1, qx, qy, qz, h, c, lanes);
    }
    if (y1 < g.ny - 1) scan_run(g, zb + (y1 + 1) * g.nx, zb + slab - 1, qx, qy, qz, h, c, lanes);
  }
  if (z1 < g.nz - 1) scan_run(g, (z1 + 1) * slab, g.nz * slab - 1, qx, qy, qz, h, c, lanes);
}

// One query (include/s3k.h).  cost may be null.  The hit is reduced over the
// lanes before every decision, so every lane takes the same path.
template <class L = Serial>
S3K_HD Hit search(const Grid& g, float qxf, float qyf, float qzf, double max_dist, Cost* cost,
                  const L& lanes = L()) {
  Hit h{(double)INFINITY, kNoIndex};
  Cost c{0, 0, 0, false};
  const int64_t kept = (int64_t)g.start[cells_of(g)];
  if (finite3(qxf, qyf, qzf) && kept > 0) {
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    const int32_t cx = cell_axis(qxf, g.ox, g.cell, g.nx), cy = cell_axis(qyf, g.oy, g.cell, g.ny),
                  cz = cell_axis(qzf, g.oz, g.cell, g.nz);
    const int32_t reach = imax(imax(imax(cx, g.nx - 1 - cx), imax(cy, g.ny - 1 - cy)),
                               imax(cz, g.nz - 1 - cz));
    const int64_t lines = (int64_t)g.ny * g.nz;
    for (int32_t r = 0;; ++r) {
      const int32_t x0 = imax(cx - r, 0), x1 = imin(cx + r, g.nx - 1);
      const int32_t y0 = imax(cy - r, 0), y1 = imin(cy + r, g.ny - 1);
      const int32_t z0 = imax(cz - r, 0), z1 = imin(cz + r, g.nz - 1);
      for (int32_t z = z0; z <= z1; ++z) {
        const bool zface = z - cz == r || cz - z == r;
        for (int32_t y = y0; y <= y1; ++y) {
          const int32_t b = (z * g.ny + y) * g.nx;
          if (zface || y - cy == r || cy - y == r) {
            scan_run(g, b + x0, b + x1, qx, qy, qz, h, c, lanes);
          } else {
            if (cx - r >= 0) scan_run(g, b + cx - r, b + cx - r, qx, qy, qz, h, c, lanes);
            if (cx + r <= g.nx - 1) scan_run(g, b + cx + r, b + cx + r, qx, qy, qz, h, c, lanes);
          }
        }
      }
      lanes.reduce(h);
      c.rings = r + 1;
      if (r >= reach) break;
      if (ring_done(h.d2, r, g.cell)) break;
      if (ring_past(r, g.cell, max_dist)) break;
      if (c.cells >= (kept - c.rows) + lines) {
        c.linear = true;
        scan_rest(g, x0, x1, y0, y1, z0, z1, qx, qy, qz, h, c, lanes);
        lanes.reduce(h);
        break;
      }
    }
  }
  if (!(h.d2 <= max_dist * max_dist)) h.i = kNoIndex;
  if (h.i == kNoIndex) {
    h.i = -1;
    h.d2 = (double)INFINITY;
  }
  if (cost) *cost = c;
  return h;
}

// ---------------------------------------------------- k nearest rows ----
// The best rows seen so far in ascending (d2, i) order, a total order; an
// empty slot is (+inf, kNoIndex) and sorts after every row.  CAP is a
// compile-time constant and every access below is a static index of an
// unrolled loop, so the slots stay in registers.  All CAP slots are kept
// sorted whatever k is: the first k of the best CAP are the best k.
template <int CAP>
struct HitK {
  double d2[CAP];
  int32_t i[CAP];
};

// what a row of the k-nearest outputs holds beside its slots
struct RowStats {
  float mean_d, mean_d2;
  int32_t filled;
};

S3K_HD bool before(double d2, int32_t i, double e2, int32_t j) {
  return d2 < e2 || (d2 == e2 && i < j);
}

template <int CAP>
S3K_HD void clear_k(HitK<CAP>& h) {
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    h.d2[s] = (double)INFINITY;
    h.i[s] = kNoIndex;
  }
}

// slot k - 1, the worst of the k kept: what a candidate has to beat
template <int CAP>
S3K_HD void worst_of(const HitK<CAP>& h, int32_t k, double& d2, int32_t& i) {
  d2 = h.d2[CAP - 1];
  i = h.i[CAP - 1];
#pragma unroll
  for (int s = 0; s < CAP - 1; ++s)
    if (s == k - 1) {
      d2 = h.d2[s];
      i = h.i[s];
    }
}

// put (d2, i) in its place; the slots after it move down one, the last is lost
template <int CAP>
S3K_HD void insert_k(HitK<CAP>& h, double d2, int32_t i) {
#pragma unroll
  for (int s = CAP - 1; s >= 0; --s) {
    // slot s - 1 still holds its old value here
    if (before(d2, i, h.d2[s], h.i[s])) {
      const bool up = s > 0 && before(d2, i, h.d2[s > 0 ? s - 1 : 0], h.i[s > 0 ? s - 1 : 0]);
      h.d2[s] = up ? h.d2[s > 0 ? s - 1 : 0] : d2;
      h.i[s] = up ? h.i[s > 0 ? s - 1 : 0] : i;
    }
  }
}

// the records of cells id0 .. id1; rows past the limit and row `self` do not count
template <int CAP>
S3K_HD void scan_run_k(const Grid& g, int32_t id0, int32_t id1, double qx, double qy, double qz,
                       int32_t k, int32_t self, double limit, HitK<CAP>& h, double& w_d2,
                       int32_t& w_i, Cost& c) {
  const uint32_t a = g.start[id0], b = g.start[id1 + 1];
  c.cells += id1 - id0 + 1;
  c.rows += b - a;
  for (uint32_t t = a; t < b; ++t) {
    const Rec r = g.rec[t];
    const double d2 = dist2(qx, qy, qz, r.x, r.y, r.z);
    if (r.i != self && d2 <= limit && before(d2, r.i, w_d2, w_i)) {
      insert_k(h, d2, r.i);
      worst_of(h, k, w_d2, w_i);
    }
  }
}

// everything outside the cube [x0, x1] x [y0, y1] x [z0, z1] of cells (scan_rest's runs)
template <int CAP>
S3K_HD void scan_rest_k(const Grid& g, int32_t x0, int32_t x1, int32_t y0, int32_t y1, int32_t z0,
                        int32_t z1, double qx, double qy, double qz, int32_t k, int32_t self,
                        double limit, HitK<CAP>& h, double& w_d2, int32_t& w_i, Cost& c) {
#define S3K_RUN(A, B) scan_run_k(g, A, B, qx, qy, qz, k, self, limit, h, w_d2, w_i, c)
  const int32_t slab = g.nx * g.ny;
  if (z0 > 0) S3K_RUN(0, z0 * slab - 1);
  for (int32_t z = z0; z <= z1; ++z) {
    const int32_t zb = z * slab;
    if (y0 > 0) S3K_RUN(zb, zb + y0 * g.nx - 1);
    for (int32_t y = y0; y <= y1; ++y) {
      const int32_t b = zb + y * g.nx;
      if (x0 > 0) S3K_RUN(b, b + x0 - 1);
      if (x1 < g.nx - 1) S3K_RUN(b + x1 + 1, b + g.nx - 1);
    }
    if (y1 < g.ny - 1) S3K_RUN(zb + (y1 + 1) * g.nx, zb + slab - 1);
  }
  if (z1 < g.nz - 1) S3K_RUN((z1 + 1) * slab, g.nz * slab - 1);
}

// One k-nearest query (include/s3k.h), 1 <= k <= CAP: search()'s walk with k
// slots.  self: the reference row that does not count (-1: none).  After
// ring r an unvisited row is at least r cell (1 - 2^-20) away (the argument
// at the head of this file, which no property of the winner enters), so once
// slot k - 1 is filled and strictly nearer than that, no unvisited row can
// come before it, a tie included.  cost may be null.
template <int CAP>
S3K_HD void search_k(const Grid& g, float qxf, float qyf, float qzf, int32_t k, int32_t self,
                     double max_dist, HitK<CAP>& h, Cost* cost) {
  clear_k(h);
  Cost c{0, 0, 0, false};
  double w_d2 = (double)INFINITY;
  int32_t w_i = kNoIndex;
  const double limit = max_dist * max_dist;
  const int64_t kept = (int64_t)g.start[cells_of(g)];
  if (finite3(qxf, qyf, qzf) && kept > 0) {
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    const int32_t cx = cell_axis(qxf, g.ox, g.cell, g.nx), cy = cell_axis(qyf, g.oy, g.cell, g.ny),
                  cz = cell_axis(qzf, g.oz, g.cell, g.nz);
    const int32_t reach = imax(imax(imax(cx, g.nx - 1 - cx), imax(cy, g.ny - 1 - cy)),
                               imax(cz, g.nz - 1 - cz));
    const int64_t lines = (int64_t)g.ny * g.nz;
    for (int32_t r = 0;; ++r) {
      const int32_t x0 = imax(cx - r, 0), x1 = imin(cx + r, g.nx - 1);
      const int32_t y0 = imax(cy - r, 0), y1 = imin(cy + r, g.ny - 1);
      const int32_t z0 = imax(cz - r, 0), z1 = imin(cz + r, g.nz - 1);
      for (int32_t z = z0; z <= z1; ++z) {
        const bool zface = z - cz == r || cz - z == r;
        for (int32_t y = y0; y <= y1; ++y) {
          const int32_t b = (z * g.ny + y) * g.nx;
          if (zface || y - cy == r || cy - y == r) {
            S3K_RUN(b + x0, b + x1);
          } else {
            if (cx - r >= 0) S3K_RUN(b + cx - r, b + cx - r);
            if (cx + r <= g.nx - 1) S3K_RUN(b + cx + r, b + cx + r);
          }
        }
      }
      c.rings = r + 1;
      if (r >= reach) break;
      // an empty slot k - 1 is +inf: never done
      if (ring_done(w_d2, r, g.cell)) break;
      if (ring_past(r, g.cell, max_dist)) break;
      if (c.cells >= (kept - c.rows) + lines) {
        c.linear = true;
        scan_rest_k(g, x0, x1, y0, y1, z0, z1, qx, qy, qz, k, self, limit, h, w_d2, w_i, c);
        break;
      }
    }
  }
#undef S3K_RUN
  if (cost) *cost = c;
}

// Write a query's row: slots 0 .. k - 1 to idx / dist (each null or the row's
// k entries; an empty slot is -1 / +inf) and the means over the filled slots,
// summed in slot order in double (+inf when none is filled).
template <int CAP>
S3K_HD RowStats emit_k(const HitK<CAP>& h, int32_t k, int32_t* idx, float* dist) {
  double sum_d = 0.0, sum_d2 = 0.0;
  int32_t filled = 0;
#pragma unroll
  for (int s = 0; s < CAP; ++s)
    if (s < k) {
      const bool has = h.i[s] != kNoIndex;
      const double d = sqrt(h.d2[s]);
      if (has) {
        sum_d += d;
        sum_d2 += h.d2[s];
        ++filled;
      }
      if (idx) idx[s] = has ? h.i[s] : -1;
      if (dist) dist[s] = has ? (float)d : INFINITY;
    }
  RowStats o{INFINITY, INFINITY, filled};
  if (filled > 0) {
    o.mean_d = (float)(sum_d / (double)filled);
    o.mean_d2 = (float)(sum_d2 / (double)filled);
  }
  return o;
}

// ------------------------------------------------------------- sampler ----
// area of face (a, b, c) in double; the caller has checked the indices
S3K_HD double face_area(const float* a, const float* b, const float* c) {
  const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1],
               e1z = (double)b[2] - (double)a[2];
  const double e2x = (double)c[0] - (double)a[0], e2y = (double)c[1] - (double)a[1],
               e2z = (double)c[2] - (double)a[2];
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  return 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

// the area of face f of the mesh, 0 (and *bad = true) when it does not count
S3K_HD double checked_area(const float* verts, int64_t V, const int32_t* faces, int64_t f,
                           bool* bad) {
  const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  *bad = true;
  if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return 0.0;
  const double a = face_area(verts + 3 * ia, verts + 3 * ib, verts + 3 * ic);
  if (!(a - a == 0.0)) return 0.0;
  *bad = false;
  return a;
}

S3K_HD uint64_t face_weight(double area, double a_max) {
  if (!(a_max > 0.0)) return 0ull;
  return (uint64_t)floor(area / a_max * kTwo32);
}

S3K_HD void sample_uniforms(int64_t k, uint64_t seed, double (&u)[4]) {
  uint32_t c[4] = {(uint32_t)((uint64_t)k & 0xffffffffu), (uint32_t)((uint64_t)k >> 32), 0u, 0u};
  s3d::philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = ((double)c[j] + 0.5) * (1.0 / kTwo32);
}

S3K_HD uint64_t sample_target(int64_t k, double u0, int64_t S, uint64_t Q) {
  const uint64_t t = (uint64_t)floor(((double)k + u0) / (double)S * (double)Q);
  return t < Q - 1 ? t : Q - 1;
}

// the smallest f with C[f] > t (t < C[F - 1])
S3K_HD int64_t pick_face(const uint64_t* C, int64_t F, uint64_t t) {
  int64_t lo = 0, hi = F - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (C[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

S3K_HD void place(const float* a, const float* b, const float* c, double u1, double u2,
                  float (&p)[3]) {
  const double s = sqrt(u1);
  const double wa = 1.0 - s, wb = s * (1.0 - u2), wc = s * u2;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    p[j] = (float)((wa * (double)a[j] + wb * (double)b[j]) + wc * (double)c[j]);
}

}  // namespace s3k
