/*
 * s3f.h — TSDF fusion of depth maps into a dense volume and triangle-mesh
 * extraction from it (marching tetrahedra).
 *
 * The reference has no counterpart in scope: its TSDF code lives in
 * mast3r/cloud_opt.  The definitions are this project's;
 * tests/tsdf_mesh_ref64.py restates both in numpy float64.
 *
 * Volume.  nx * ny * nz voxels, x fastest, in three planes:
 *   tsdf   float32 [nz, ny, nx], in [-1, 1]
 *   weight float32 [nz, ny, nx]
 *   rgb    float32 [3, nz, ny, nx]
 * with origin[3] (world position of the centre of voxel (0,0,0)), voxel and
 * trunc (world units, both > 0) and w_max > 0, all float32.  A fresh volume
 * is tsdf = 1, weight = 0, rgb = 0.  The centre of voxel (i, j, k) is
 * x_w = origin + voxel * (i, j, k), evaluated in double.
 *
 * Integration (s3f_integrate), V views in one launch.  View v has
 *   depth [H, W]     float32 z-depth in the view's camera units
 *   color [3, H, W]  float32, optional (null: the rgb plane is not touched)
 *   wmap  [H, W]     float32 per-pixel weight, optional (null: 1)
 *   K [9]            row-major pixel intrinsics; only fx = K[0], fy = K[4],
 *                    cx = K[2], cy = K[5] are read.  Integer pixel indices
 *                    are pixel centres (the convention of s3c.h).
 *   T_WC [16]        row-major camera-to-world similarity (s R | t): s is the
 *                    norm of the first column of the 3x3 block M = s R.
 * A view is valid iff fx, fy, cx, cy and the 12 entries of (M | t) are finite,
 * fx > 0, fy > 0 and s > 0 (s finite); an invalid view is skipped for every
 * voxel.  Per voxel centre x_w, the views taken in index order:
 *   1. x_c = M^T (x_w - t) / s^2  (= R^T (x_w - t) / s), z = x_c.z;
 *      skip unless z > 0
 *   2. u = fx x_c.x / z + cx, v = fy x_c.y / z + cy
 *   3. (a, b) = (floor(u + 0.5), floor(v + 0.5)); skip unless
 *      0 <= a <= W - 1 and 0 <= b <= H - 1, compared as doubles before
 *      anything becomes an index (a NaN fails)
 *   4. d = depth[b, a]; skip unless d is finite and > 0
 *   5. w_o = wmap[b, a] (1 without a map); skip unless finite and > 0
 *   6. sdf = s (d - z); skip if sdf < -trunc
 *   7. f_o = min(1, sdf / trunc)
 *   8. tsdf <- (tsdf w + f_o w_o) / (w + w_o), and with colour each channel
 *      rgb_c <- (rgb_c w + color[c, b, a] w_o) / (w + w_o)
 *   9. w <- min(w + w_o, w_max)
 * Arithmetic (csrc/tsdf_mesh_math.hpp, host + device, -ffp-contract=off):
 * everything in double on the float32 inputs; tsdf, weight and rgb are
 * rounded to float32 once after every view.  A voxel is a pure function of
 * its own state and the views: no atomics, no dependence on the launch
 * geometry, a batch of V views is bit-identical to V single-view calls in
 * the same order, and a voxel no view updates keeps its bits (it is not
 * written).  The volume is read and written once per call; a one-thread-per-
 * view prologue writes the inverse transforms into the workspace.
 *
 * Extraction (s3f_mesh_count, then s3f_mesh_emit): marching tetrahedra on the
 * lattice of voxel centres.
 *   cell      (i, j, k), i < nx-1, j < ny-1, k < nz-1, has the 8 lattice points
 *             i..i+1, j..j+1, k..k+1; it is valid iff all 8 have
 *             weight >= w_min (w_min > 0).  Cell index = i + nx (j + ny k).
 *   split     a valid cell is cut into the 6 Kuhn tetrahedra: corners
 *             000, e_a, e_a + e_b, 111 for the permutations (a, b, c) of the
 *             axes in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx.
 *   inside    a lattice point is inside iff tsdf < 0 (0 and NaN are outside).
 *   edges     a lattice point p = (x, y, z) owns 7 edges p -> p + dir[d],
 *             dir = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (0,1,1), (1,0,1),
 *             (1,1,1); edge id e = 7 (x + nx (y + ny z)) + d.  Every edge of
 *             every tetrahedron is such an edge.
 *   vertices  an edge has a vertex iff its ends differ in insideness and it
 *             is an edge of at least one valid cell.  Vertices are numbered
 *             by ascending edge id.  With a = p, b = p + dir[d]:
 *               t = f_a / (f_a - f_b)
 *               position = origin + voxel (p + t dir[d])
 *               colour   = c_a + t (c_b - c_a)
 *             in double, rounded to float32 once.
 *   triangles a tetrahedron with 1 or 3 inside corners gives one triangle,
 *             one with 2 gives a quad (corners a, b on one side, c, d on the
 *             other, each pair in corner order: the cycle ac, ad, bd, bc),
 *             split into two triangles fanned from its vertex of smallest
 *             edge id, cycle order kept.  Every triangle is wound so that
 *             its normal (right-hand rule) points to the outside corners
 *             (tsdf >= 0, free space).  Triangles are ordered by cell index,
 *             then tetrahedron, then the fan order.
 * Outputs: verts [nv, 3] float32, vcol [nv, 3] float32, faces [nt, 3] int32.
 * Everything is integer counting and exclusive scans: the output is a
 * function of the volume alone.  A lattice value of exactly 0 gives
 * coincident vertices and zero-area triangles; that is not repaired.
 */
#ifndef S3F_H
#define S3F_H
#include "s3_common.h"

#define S3F_VIEW_DOUBLES 20

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace s3f_integrate needs for n_views views (0 for
 * n_views <= 0): S3F_VIEW_DOUBLES doubles each. */
size_t s3f_integrate_workspace_bytes(int32_t n_views);

/* Fuse n_views views into the volume (definition above).  All pointers are
 * device memory: depth [V, H, W], color [V, 3, H, W] or null, wmap [V, H, W]
 * or null, K [V, 9], T_WC [V, 16]; workspace 8-byte aligned.  Returns
 * S3_ERR_INVALID before any device work for non-positive dims or image size,
 * 7 nx ny nz >= 2^31, H W >= 2^31, voxel, trunc or w_max not finite and > 0,
 * n_views <= 0 or a workspace that is too small.  Two stream-ordered
 * launches, no host read. */
int s3f_integrate(float* tsdf, float* weight, float* rgb, int32_t nx, int32_t ny, int32_t nz,
                  float ox, float oy, float oz, float voxel, float trunc, float w_max,
                  const float* depth, const float* color, const float* wmap, const float* K,
                  const float* T_WC, int32_t n_views, int32_t H, int32_t W, void* workspace,
                  size_t workspace_bytes, void* stream);

/* Bytes of the workspace the two extraction calls share (0 when a dimension is
 * not positive or 7 nx ny nz >= 2^31): 6 bytes per voxel plus the block sums. */
size_t s3f_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);

/* Phase 1: classify cells and edges, scan.  counts: device int64 [2], written
 * with {vertices, triangles}.  The workspace (8-byte aligned) carries the
 * result to s3f_mesh_emit and must not be touched in between.  A dimension
 * of 1 gives counts {0, 0}.  S3_ERR_INVALID before any device work for
 * non-positive dims, 7 nx ny nz >= 2^31, w_min not finite and > 0 or a
 * workspace that is too small. */
int s3f_mesh_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz,
                   float w_min, int64_t* counts, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Phase 2: write the mesh of the volume s3f_mesh_count classified.  n_verts
 * and n_tris are the two counts the host read; verts and vcol [verts_cap, 3]
 * float32, faces [faces_cap, 3] int32 (any may be null when its count is 0).
 * rgb may be null: vcol is then not written.  Every store is bounded by the
 * two counts.  S3_ERR_INVALID before any device work when verts_cap < n_verts,
 * faces_cap < n_tris, a count is negative or exceeds what the volume can
 * hold, or the workspace is too small. */
int s3f_mesh_emit(const float* tsdf, const float* rgb, int32_t nx, int32_t ny, int32_t nz, float ox,
                  float oy, float oz, float voxel, int64_t n_verts, int64_t n_tris, float* verts,
                  float* vcol, int32_t* faces, int64_t verts_cap, int64_t faces_cap,
                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3F_H */
