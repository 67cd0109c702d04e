// TSDF fusion and marching-tetrahedra extraction (include/s3f.h); the
// arithmetic is tsdf_mesh_math.hpp.
//
//   k_tsdf_views      one thread per view: K and T_WC in, the 20-double view
//                     record (flag, M^T / s^2, t, s, fx, fy, cx, cy) out.
//   k_tsdf_integrate  one voxel per thread: its tsdf, weight and colour are
//                     loaded once, every view of the batch is applied in
//                     index order with the state rounded to float32 after
//                     each, and the voxel is stored once if any view updated
//                     it.  The view records are read at wave-uniform
//                     addresses.
//   k_mesh_cells      one cell per thread: 8 weights, 8 signs -> the cell's
//                     triangle count (0 for an invalid cell), one byte.
//   k_mesh_edges      one lattice point per thread: the 7-bit mask of its
//                     edges that carry a vertex (ends differ in sign and a
//                     cell around the edge has triangles, which is the same
//                     as being valid); per-workgroup sums of both counts.
//   k_mesh_scan       one workgroup: exclusive scan of the workgroup sums in
//                     place, the two totals to `counts`.
//   k_mesh_verts      one lattice point per thread: in-workgroup scan + the
//                     workgroup's base -> the index of its first vertex
//                     (kept for k_mesh_tris), then its vertices.
//   k_mesh_tris       one cell per thread: the same scan on the triangle
//                     counts, then its triangles, the vertex of an edge found
//                     through the owner's base and mask.
//
// Integer counts and scans only, no atomic: the mesh is a function of the
// volume alone.
#include "common.hpp"
#include "s3f.h"
#include "tsdf_mesh_math.hpp"
#include "wave_scan.hpp"

namespace {

constexpr int kT = 256;
constexpr int kScanT = 1024;
constexpr int kView = s3f::kView;
static_assert(kView == S3F_VIEW_DOUBLES, "view record size");
using u32 = unsigned int;
using u8 = unsigned char;

struct Dims {
  int32_t nx, ny, nz;
  int64_t n;   // nx * ny * nz
};

__global__ void __launch_bounds__(64)
k_tsdf_views(const float* __restrict__ K, const float* __restrict__ T, int32_t V,
             double* __restrict__ views) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= V) return;
  float k[9], t[16];
#pragma unroll
  for (int j = 0; j < 9; ++j) k[j] = K[v * 9 + j];
#pragma unroll
  for (int j = 0; j < 16; ++j) t[j] = T[v * 16 + j];
  double vw[kView];
  s3f::prepare_view(k, t, vw);
#pragma unroll
  for (int j = 0; j < kView; ++j) views[(int64_t)v * kView + j] = vw[j];
}

__global__ void __launch_bounds__(kT)
k_tsdf_integrate(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ rgb,
                 Dims dm, float ox, float oy, float oz, float voxel, float trunc, float w_max,
                 const float* __restrict__ depth, const float* __restrict__ color,
                 const float* __restrict__ wmap, const double* __restrict__ views, int32_t V,
                 int32_t H, int32_t W) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= dm.n) return;
  const int i = (int)(p % dm.nx);
  const int64_t r = p / dm.nx;
  const int j = (int)(r % dm.ny), k = (int)(r / dm.ny);
  double xw[3];
  s3f::voxel_centre(ox, oy, oz, voxel, i, j, k, xw);
  float f = tsdf[p], w = weight[p];
  float c[3] = {0.f, 0.f, 0.f};
  if (color) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = rgb[ch * dm.n + p];
  }
  const int64_t plane = (int64_t)H * W;
  bool any = false;
  for (int v = 0; v < V; ++v) {
    const bool hit = s3f::integrate_view(views + (int64_t)v * kView, xw, H, W, depth + v * plane,
                                         color ? color + v * 3 * plane : nullptr,
                                         wmap ? wmap + v * plane : nullptr, trunc, w_max, f, w, c);
    any = any || hit;
  }
  if (!any) return;
  tsdf[p] = f;
  weight[p] = w;
  if (color) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch * dm.n + p] = c[ch];
  }
}

// ------------------------------------------------------------ extraction ---
struct MeshWs {
  u8* cell_tris;    // [n]
  u8* vert_mask;    // [n]
  u32* vbase;       // [n]
  u32* vblock;      // [blocks]
  u32* tblock;      // [blocks]
};

size_t mesh_ws_bytes(int64_t n) {
  const int64_t blocks = s3::cdiv(n, kT);
  return (size_t)(((2 * n + 7) / 8) * 8 + 4 * n + 8 * blocks);
}

MeshWs mesh_ws(void* ws, int64_t n) {
  const int64_t blocks = s3::cdiv(n, kT);
  u8* b = static_cast<u8*>(ws);
  MeshWs m;
  m.cell_tris = b;
  m.vert_mask = b + n;
  m.vbase = reinterpret_cast<u32*>(b + ((2 * n + 7) / 8) * 8);
  m.vblock = m.vbase + n;
  m.tblock = m.vblock + blocks;
  return m;
}

__device__ __forceinline__ void split(int64_t p, const Dims& dm, int& i, int& j, int& k) {
  i = (int)(p % dm.nx);
  const int64_t r = p / dm.nx;
  j = (int)(r % dm.ny);
  k = (int)(r / dm.ny);
}

// The 8-bit insideness mask of the cell at lattice point p (corner code
// dx + 2 dy + 4 dz); the caller guarantees the cell is in range.
__device__ __forceinline__ unsigned cell_inside(const float* __restrict__ tsdf, int64_t p,
                                                int64_t nx, int64_t nxny) {
  unsigned m = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float f = tsdf[p + (c & 1) + nx * ((c >> 1) & 1) + nxny * ((c >> 2) & 1)];
    m |= (f < 0.0f ? 1u : 0u) << c;
  }
  return m;
}

__global__ void __launch_bounds__(kT)
k_mesh_cells(const float* __restrict__ tsdf, const float* __restrict__ weight, Dims dm,
             float w_min, u8* __restrict__ cell_tris) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= dm.n) return;
  int i, j, k;
  split(p, dm, i, j, k);
  int nt = 0;
  if (i < dm.nx - 1 && j < dm.ny - 1 && k < dm.nz - 1) {
    const int64_t nx = dm.nx, nxny = nx * dm.ny;
    bool valid = true;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      valid = valid && weight[p + (c & 1) + nx * ((c >> 1) & 1) + nxny * ((c >> 2) & 1)] >= w_min;
    if (valid) nt = s3f::cell_triangles(cell_inside(tsdf, p, nx, nxny));
  }
  cell_tris[p] = (u8)nt;
}

__global__ void __launch_bounds__(kT)
k_mesh_edges(const float* __restrict__ tsdf, Dims dm, MeshWs ws) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int64_t nx = dm.nx, nxny = nx * dm.ny;
  u32 mask = 0, nt = 0;
  if (p < dm.n) {
    int x[3];
    split(p, dm, x[0], x[1], x[2]);
    const int dim[3] = {dm.nx, dm.ny, dm.nz};
    const int64_t stride[3] = {1, nx, nxny};
    const bool in_p = tsdf[p] < 0.0f;
    nt = ws.cell_tris[p];
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      const int code = s3f::dir_code(d);
      bool ok = true;
      int64_t q = p;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if ((code >> a) & 1) {
          ok = ok && x[a] + 1 < dim[a];
          q += stride[a];
        }
      }
      if (!ok) continue;
      if ((tsdf[q] < 0.0f) == in_p) continue;
      // the cells around the edge: p - o, o free on the axes the edge does
      // not advance along
      bool live = false;
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        if (o & code) continue;
        bool in_range = true;
        int64_t cell = p;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int ca = x[a] - ((o >> a) & 1);
          in_range = in_range && ca >= 0 && ca < dim[a] - 1;
          cell -= stride[a] * ((o >> a) & 1);
        }
        if (in_range && ws.cell_tris[cell] != 0) live = true;
      }
      if (live) mask |= 1u << d;
    }
    ws.vert_mask[p] = (u8)mask;
  }
  __shared__ u32 s_w[kT / 64];
  u32 vsum, tsum;
  s3::block_excl_add<kT>((u32)__popc(mask), s_w, &vsum);
  s3::block_excl_add<kT>(nt, s_w, &tsum);
  if (threadIdx.x == 0) {
    ws.vblock[blockIdx.x] = vsum;
    ws.tblock[blockIdx.x] = tsum;
  }
}

__global__ void __launch_bounds__(kScanT)
k_mesh_scan(u32* __restrict__ vblock, u32* __restrict__ tblock, int64_t blocks,
            int64_t* __restrict__ counts) {
  // This one workgroup makes hundreds of serial trips of two scans.  It keeps
  // its own workgroup step: the barrier that frees s_w stands in front of the
  // write, where the waves reach it after their wave scan, and not behind the
  // read as in s3::block_excl_add (measured 2.5 % slower here).
  __shared__ u32 s_w[kScanT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto excl_add = [&](u32 x, u32& total) {
    const u32 inc = s3::wave_incl_add(x, lane);
    __syncthreads();   // s_w of the scan before has been read
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u32 before = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < kScanT / 64; ++k) {
      const u32 s = s_w[k];
      if (k < wave) before += s;
      sum += s;
    }
    total = sum;
    return before + inc - x;
  };
  unsigned long long carry_v = 0, carry_t = 0;
  for (int64_t base = 0; base < blocks; base += kScanT) {
    const int64_t b = base + threadIdx.x;
    const u32 v = b < blocks ? vblock[b] : 0u, t = b < blocks ? tblock[b] : 0u;
    u32 vs, ts;
    const u32 ve = excl_add(v, vs);
    const u32 te = excl_add(t, ts);
    if (b < blocks) {
      vblock[b] = (u32)(carry_v + ve);
      tblock[b] = (u32)(carry_t + te);
    }
    carry_v += vs;
    carry_t += ts;
  }
  if (threadIdx.x == 0) {
    counts[0] = (int64_t)carry_v;
    counts[1] = (int64_t)carry_t;
  }
}

__global__ void __launch_bounds__(kT)
k_mesh_verts(const float* __restrict__ tsdf, const float* __restrict__ rgb, Dims dm, float ox,
             float oy, float oz, float voxel, MeshWs ws, int64_t n_verts,
             float* __restrict__ verts, float* __restrict__ vcol) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  const u32 mask = p < dm.n ? ws.vert_mask[p] : 0u;
  __shared__ u32 s_w[kT / 64];
  const u32 first = s3::block_excl_add<kT>((u32)__popc(mask), s_w) + ws.vblock[blockIdx.x];
  if (p >= dm.n) return;
  ws.vbase[p] = first;
  if (!mask) return;
  int i, j, k;
  split(p, dm, i, j, k);
  const int64_t nx = dm.nx, nxny = nx * dm.ny;
  const float fa = tsdf[p];
  float ca[3] = {0.f, 0.f, 0.f};
  if (rgb) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) ca[ch] = rgb[ch * dm.n + p];
  }
  int64_t idx = first;
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    if (!((mask >> d) & 1u)) continue;
    const int code = s3f::dir_code(d);
    const int64_t q = p + (code & 1) + nx * ((code >> 1) & 1) + nxny * ((code >> 2) & 1);
    float cb[3] = {0.f, 0.f, 0.f};
    if (rgb) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) cb[ch] = rgb[ch * dm.n + q];
    }
    float pos[3], col[3] = {0.f, 0.f, 0.f};
    s3f::edge_vertex(ox, oy, oz, voxel, i, j, k, d, fa, tsdf[q], rgb ? ca : nullptr,
                     rgb ? cb : nullptr, pos, col);
    if (idx < n_verts) {
#pragma unroll
      for (int a = 0; a < 3; ++a) verts[idx * 3 + a] = pos[a];
      if (rgb) {
#pragma unroll
        for (int a = 0; a < 3; ++a) vcol[idx * 3 + a] = col[a];
      }
    }
    ++idx;
  }
}

__global__ void __launch_bounds__(kT)
k_mesh_tris(const float* __restrict__ tsdf, Dims dm, MeshWs ws, int64_t n_tris,
            int32_t* __restrict__ faces) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  const u32 nt = p < dm.n ? ws.cell_tris[p] : 0u;
  __shared__ u32 s_w[kT / 64];
  const u32 first = s3::block_excl_add<kT>(nt, s_w) + ws.tblock[blockIdx.x];
  if (!nt) return;
  const int64_t nx = dm.nx, nxny = nx * dm.ny;
  const unsigned inside = cell_inside(tsdf, p, nx, nxny);   // nt > 0: the cell is in range
  int64_t idx = first;
  for (int t = 0; t < 6; ++t) {
    int64_t tri[2][3];
    const int m = s3f::tet_triangles(t, inside, p, nx, nxny, tri);
    for (int s = 0; s < m; ++s, ++idx) {
      if (idx >= n_tris) continue;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int64_t owner = tri[s][a] / 7;
        const int d = (int)(tri[s][a] % 7);
        faces[idx * 3 + a] =
            (int32_t)(ws.vbase[owner] + (u32)__popc((u32)ws.vert_mask[owner] & ((1u << d) - 1u)));
      }
    }
  }
}

bool finite_pos(float v) { return v > 0.0f && v <= 3.402823466e+38f; }

// nx ny nz > 0 and 7 nx ny nz < 2^31, without overflow.
bool dims_ok(int32_t nx, int32_t ny, int32_t nz, int64_t& n) {
  n = 0;
  if (nx <= 0 || ny <= 0 || nz <= 0) return false;
  const int64_t lim = ((int64_t)1 << 31) / 7 + 1;   // n < lim  <=>  7 n < 2^31
  const int64_t a = (int64_t)nx * ny;
  if (a >= lim) return false;
  const int64_t b = a * nz;
  if (b >= lim || 7 * b >= ((int64_t)1 << 31)) return false;
  n = b;
  return true;
}

}  // namespace

extern "C" size_t s3f_integrate_workspace_bytes(int32_t n_views) {
  if (n_views <= 0) return 0;
  return (size_t)n_views * kView * sizeof(double);
}

extern "C" int s3f_integrate(float* tsdf, float* weight, float* rgb, int32_t nx, int32_t ny,
                             int32_t nz, float ox, float oy, float oz, float voxel, float trunc,
                             float w_max, const float* depth, const float* color,
                             const float* wmap, const float* K, const float* T_WC,
                             int32_t n_views, int32_t H, int32_t W, void* workspace,
                             size_t workspace_bytes, void* stream) {
  s3::clear_error();
  Dims dm{nx, ny, nz, 0};
  S3_REQUIRE(dims_ok(nx, ny, nz, dm.n), "s3f_integrate: volume %d x %d x %d: dims must be positive "
             "and 7 nx ny nz < 2^31", nx, ny, nz);
  S3_REQUIRE(n_views > 0, "s3f_integrate: n_views <= 0");
  S3_REQUIRE(n_views <= (1 << 20), "s3f_integrate: n_views too large");
  S3_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31),
             "s3f_integrate: bad image size %d x %d", H, W);
  S3_REQUIRE(finite_pos(voxel) && finite_pos(trunc) && finite_pos(w_max),
             "s3f_integrate: voxel, trunc and w_max must be finite and > 0");
  S3_REQUIRE(ox - ox == 0.0f && oy - oy == 0.0f && oz - oz == 0.0f,
             "s3f_integrate: origin must be finite");
  S3_REQUIRE(workspace && workspace_bytes >= s3f_integrate_workspace_bytes(n_views),
             "s3f_integrate: workspace too small");
  S3_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
             "s3f_integrate: workspace must be 8-byte aligned");
  S3_REQUIRE(tsdf && weight && depth && K && T_WC, "s3f_integrate: null pointer");
  S3_REQUIRE(!color || rgb, "s3f_integrate: color given without an rgb plane");
  hipStream_t st = s3::as_stream(stream);
  double* views = static_cast<double*>(workspace);
  k_tsdf_views<<<(unsigned)s3::cdiv(n_views, 64), 64, 0, st>>>(K, T_WC, n_views, views);
  S3_LAUNCH_CHECK();
  k_tsdf_integrate<<<(unsigned)s3::cdiv(dm.n, kT), kT, 0, st>>>(
      tsdf, weight, rgb, dm, ox, oy, oz, voxel, trunc, w_max, depth, color, wmap, views, n_views,
      H, W);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" size_t s3f_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  int64_t n;
  if (!dims_ok(nx, ny, nz, n)) return 0;
  return mesh_ws_bytes(n);
}

extern "C" int s3f_mesh_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny,
                              int32_t nz, float w_min, int64_t* counts, void* workspace,
                              size_t workspace_bytes, void* stream) {
  s3::clear_error();
  Dims dm{nx, ny, nz, 0};
  S3_REQUIRE(dims_ok(nx, ny, nz, dm.n), "s3f_mesh_count: volume %d x %d x %d: dims must be "
             "positive and 7 nx ny nz < 2^31", nx, ny, nz);
  S3_REQUIRE(finite_pos(w_min), "s3f_mesh_count: w_min must be finite and > 0");
  S3_REQUIRE(workspace && workspace_bytes >= mesh_ws_bytes(dm.n),
             "s3f_mesh_count: workspace too small");
  S3_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
             "s3f_mesh_count: workspace must be 8-byte aligned");
  S3_REQUIRE(tsdf && weight && counts, "s3f_mesh_count: null pointer");
  hipStream_t st = s3::as_stream(stream);
  const MeshWs ws = mesh_ws(workspace, dm.n);
  const int64_t blocks = s3::cdiv(dm.n, kT);
  k_mesh_cells<<<(unsigned)blocks, kT, 0, st>>>(tsdf, weight, dm, w_min, ws.cell_tris);
  S3_LAUNCH_CHECK();
  k_mesh_edges<<<(unsigned)blocks, kT, 0, st>>>(tsdf, dm, ws);
  S3_LAUNCH_CHECK();
  k_mesh_scan<<<1, kScanT, 0, st>>>(ws.vblock, ws.tblock, blocks, counts);
  S3_LAUNCH_CHECK();
  return S3_OK;
}

extern "C" int s3f_mesh_emit(const float* tsdf, const float* rgb, int32_t nx, int32_t ny,
                             int32_t nz, float ox, float oy, float oz, float voxel,
                             int64_t n_verts, int64_t n_tris, float* verts, float* vcol,
                             int32_t* faces, int64_t verts_cap, int64_t faces_cap,
                             void* workspace, size_t workspace_bytes, void* stream) {
  s3::clear_error();
  Dims dm{nx, ny, nz, 0};
  S3_REQUIRE(dims_ok(nx, ny, nz, dm.n), "s3f_mesh_emit: volume %d x %d x %d: dims must be "
             "positive and 7 nx ny nz < 2^31", nx, ny, nz);
  S3_REQUIRE(n_verts >= 0 && n_verts <= 7 * dm.n && n_tris >= 0 && n_tris <= 12 * dm.n,
             "s3f_mesh_emit: counts out of range");
  S3_REQUIRE(verts_cap >= n_verts, "s3f_mesh_emit: verts capacity %lld < %lld vertices",
             (long long)verts_cap, (long long)n_verts);
  S3_REQUIRE(faces_cap >= n_tris, "s3f_mesh_emit: faces capacity %lld < %lld triangles",
             (long long)faces_cap, (long long)n_tris);
  S3_REQUIRE(workspace && workspace_bytes >= mesh_ws_bytes(dm.n),
             "s3f_mesh_emit: workspace too small");
  S3_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
             "s3f_mesh_emit: workspace must be 8-byte aligned");
  S3_REQUIRE(tsdf, "s3f_mesh_emit: null pointer");
  S3_REQUIRE(n_verts == 0 || (verts && (!rgb || vcol)), "s3f_mesh_emit: null vertex output");
  S3_REQUIRE(n_tris == 0 || faces, "s3f_mesh_emit: null face output");
  S3_REQUIRE(finite_pos(voxel), "s3f_mesh_emit: voxel must be finite and > 0");
  if (n_verts == 0 && n_tris == 0) return S3_OK;
  hipStream_t st = s3::as_stream(stream);
  const MeshWs ws = mesh_ws(workspace, dm.n);
  const int64_t blocks = s3::cdiv(dm.n, kT);
  k_mesh_verts<<<(unsigned)blocks, kT, 0, st>>>(tsdf, rgb, dm, ox, oy, oz, voxel, ws, n_verts,
                                                verts, vcol);
  S3_LAUNCH_CHECK();
  k_mesh_tris<<<(unsigned)blocks, kT, 0, st>>>(tsdf, dm, ws, n_tris, faces);
  S3_LAUNCH_CHECK();
  return S3_OK;
}
