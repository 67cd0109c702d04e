/*
 * s3k.h — exact nearest neighbour on a uniform grid, distance statistics and
 * area-uniform mesh sampling: what the geometry scores of evaluate.py
 * (accuracy, completion, Chamfer distance, F-score) are reductions of.
 *
 * The reference has no counterpart (it scores no geometry; its trajectory
 * error comes from the evo package).  The definitions are this project's;
 * tests/nn_search_ref64.py restates them in numpy float64 and
 * csrc/nn_search_math.hpp holds the arithmetic, host + device.
 *
 * Grid (s3k_grid_build).  ref [n, 3] float32, n < 2^31; origin[3] (host
 * doubles, finite), cell (double, finite, > 0), dims nx, ny, nz >= 1 with
 * nx ny nz <= 2^27.  Per axis
 *   c = clamp(floor(((double)x - origin) / cell), 0, dim - 1)
 * clamped as a double before it becomes an integer (any finite float32 is
 * safe); flat cell id = (cz ny + cy) nx + cx.  A row with a non-finite
 * coordinate is left out, counted in *dropped, and is never returned.  The
 * grid is: start [cells + 1] uint32 (exclusive sums of the cells' counts,
 * start[cells] = kept rows) and one 16-byte record (x, y, z, index) per kept
 * row, the records of a cell contiguous.  The order of the records inside a
 * cell is not defined (the counts and slots are integer atomics); no result
 * depends on it.
 *
 * Query (s3k_query).  q [m, 3] float32 -> idx [m] int32, dist [m] float32.
 * Over the kept rows i, with dx = (double)q_x - (double)r_x and so on,
 *   d2_i = (dx dx + dy dy) + dz dz          (each product and sum rounds once)
 * the winner is the smallest d2, ties to the smallest i; dist =
 * (float)sqrt(d2).  max_dist is a double >= 0 or +inf: the winner counts only
 * if d2 <= max_dist max_dist.  idx = -1 and dist = +inf when no row
 * qualifies, the reference is empty or the query row is not finite.  The
 * result is bit for bit that of a scan of every row, whatever the grid.
 *
 * Search.  The query's cell is clamped like a row's; cells are visited in
 * Chebyshev rings r = 0, 1, 2, ... around it, each intersected with the grid.
 * After ring r the search stops when
 *   best_d2 < (r cell (1 - 2^-20))^2
 * (a row in a cell of ring > r is at least r cells away on some axis, rows
 * and queries outside the grid included, since clamping only moves a cell
 * towards the query's; the factor covers the rounding of the cell
 * assignment), when r cell (1 - 2^-20) > max_dist, or when the rings cover
 * the grid.  When the cells visited so far reach the rows not yet visited
 * plus ny nz, the rest of the records is scanned linearly instead (the slabs
 * and rows outside the visited cube as contiguous runs): a query visits no
 * cell and no row twice.  Queries are processed in the order of their cell
 * (one radix sort of the cell ids, csrc/radix_pass.hpp) and written back to
 * their own positions; one thread per query.
 *
 * k nearest (s3k_knn).  q [m, 3] float32, 1 <= k <= 32 -> idx [m, k] int32,
 * dist [m, k] float32, mean_d [m], mean_d2 [m] float32; each output may be
 * null, not all four.  The candidates of query j are the kept rows i, without
 * row i = j when exclude_self is set (by index alone: the caller's promise
 * that q is ref, so m <= n); d2_i as above, and a candidate counts only if
 * d2 <= max_dist max_dist.  The row holds the first min(k, candidates)
 * candidates in ascending (d2, i) order, a total order: slot s has the index
 * i_s and dist = (float)sqrt(d2_s); an unfilled slot has -1 and +inf, and a
 * non-finite query row fills none.  With c filled slots, summed in slot
 * order in double,
 *   mean_d  = (float)((sum_s sqrt(d2_s)) / c)   (the double root, not dist)
 *   mean_d2 = (float)((sum_s d2_s) / c)
 * and +inf for both when c = 0.  The result is bit for bit that of sorting
 * every row, whatever the grid.  The walk is the query's, with the stop rule
 * on slot k - 1: after ring r it stops when k slots are filled and
 *   d2_{k-1} < (r cell (1 - 2^-20))^2,
 * strict, so a row that ties with the k-th is never given up; the other two
 * stops and the linear rest are unchanged, and a query visits no cell and no
 * row twice.  One thread per query in cell order; the k slots live in
 * registers (4, 8, 16 or 32 of them, the fewest that hold k).
 * s3k_set_query_mode does not apply.
 *
 * Statistics (s3k_dist_stats).  Over the finite entries of dist [m]:
 *   out[0] their count, out[1] sum d, out[2] sum d d, out[3] the count of
 *   d <= threshold, out[4] the maximum (-inf when there is none)
 * as doubles.  Workgroup b sums entries [2048 b, 2048 b + 2048): thread t its
 * 8 consecutive entries in order, then a pairwise tree over the threads; one
 * workgroup then adds the partials in index order per thread and the same
 * tree.  The order is a function of m alone: no atomics, two calls give the
 * same bits.
 *
 * Sampling (s3k_sample_mesh).  verts [V, 3] float32, faces [F, 3] int32,
 * F < 2^31, S samples, a 64-bit seed -> points [S, 3] float32, face [S]
 * int32, and device counters bad, total (int64 each).
 *   e1 = b - a, e2 = c - a, n = e1 x e2 (n_x = e1_y e2_z - e1_z e2_y, ...),
 *   area_f = 0.5 sqrt((n_x n_x + n_y n_y) + n_z n_z)         in double;
 * a face with an index outside [0, V) or a non-finite area has area 0 and is
 * counted in *bad.  A_max = max_f area_f;
 *   w_f = (uint64)floor(area_f / A_max 2^32)  (0 when A_max = 0),
 * C_f the inclusive sum of w (exact, uint64), Q = C_{F-1} -> *total.  With
 * Q = 0 (or F = 0) nothing else is written.  Sample k: Philox4x32-10 with
 * counter (k lo32, k hi32, 0, 0), key (seed lo32, seed hi32) -> x_0..3;
 *   u_j = ((double)x_j + 0.5) 2^-32
 *   t = min((uint64)floor(((double)k + u_0) / (double)S (double)Q), Q - 1)
 *   face = the smallest f with C_f > t;  s = sqrt(u_1)
 *   point = ((1 - s) a + (s (1 - u_2)) b) + (s u_2) c
 * per coordinate in double, rounded to float32 once: one stratified sample
 * per stratum of Q / S, so |n_f - S w_f / Q| < 2 for every face.
 *
 * Every entry point is stream-ordered, reads nothing back to the host and
 * allocates nothing: the workspaces are the caller's (256-byte aligned).
 * Arguments are checked before any device work (S3_ERR_INVALID, message in
 * s3_last_error()).  No floating-point atomic anywhere.
 */
#ifndef S3K_H
#define S3K_H
#include "s3_common.h"

#define S3K_MAX_CELLS (1 << 27)
#define S3K_MAX_K 32

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of a grid of n rows and nx ny nz cells (0 for n < 0, n > 2^31 - 2048,
 * a dimension < 1 or more than S3K_MAX_CELLS cells): start, the records and
 * the build's scratch. */
size_t s3k_grid_workspace_bytes(int64_t n, int32_t nx, int32_t ny, int32_t nz);

/* Build the grid of ref [n, 3] (device) into `grid` (device, 256-byte
 * aligned, grid_bytes >= s3k_grid_workspace_bytes); origin: host double[3].
 * dropped: device int64, written.  n = 0 gives an empty grid (ref may be
 * null). */
int s3k_grid_build(const float* ref, int64_t n, const double* origin, double cell, int32_t nx,
                   int32_t ny, int32_t nz, void* grid, size_t grid_bytes, int64_t* dropped,
                   void* stream);

/* Bytes of the workspace of a query of m rows (0 for m <= 0 or
 * m > 2^31 - 2048): the sort's key and index columns and histograms. */
size_t s3k_query_workspace_bytes(int64_t m);

/* Nearest row of the grid (built with the same n, origin, cell, dims) for
 * each of q [m, 3] (device): idx [m] int32, dist [m] float32 (device).
 * m = 0 does nothing. */
int s3k_query(const void* grid, size_t grid_bytes, int64_t n, const double* origin, double cell,
              int32_t nx, int32_t ny, int32_t nz, const float* q, int64_t m, double max_dist,
              int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of the workspace of s3k_knn over m rows (0 for m <= 0 or
 * m > 2^31 - 2048): the sort's columns and histograms. */
size_t s3k_knn_workspace_bytes(int64_t m);

/* The k nearest rows of the grid (built with the same n, origin, cell, dims)
 * for each of q [m, 3] (device), 1 <= k <= S3K_MAX_K: idx [m, k] int32,
 * dist [m, k], mean_d [m], mean_d2 [m] float32 (device; each may be null,
 * not all).  exclude_self != 0: row j is no candidate of query j (m <= n).
 * m = 0 does nothing. */
int s3k_knn(const void* grid, size_t grid_bytes, int64_t n, const double* origin, double cell,
            int32_t nx, int32_t ny, int32_t nz, const float* q, int64_t m, int32_t k,
            int32_t exclude_self, double max_dist, int32_t* idx, float* dist, float* mean_d,
            float* mean_d2, void* workspace, size_t workspace_bytes, void* stream);

/* How s3k_query walks (process-wide; for measurements, every mode returns
 * the same bits): 0 queries sorted by cell, one thread each (the default);
 * 1 the queries' own order, one thread each; 2 sorted, one wave each.  Any
 * other value is 0. */
void s3k_set_query_mode(int32_t mode);

/* Bytes of the workspace of s3k_dist_stats over m entries (0 for m <= 0 or
 * m > (2^31 - 1) 2048, which s3k_dist_stats rejects). */
size_t s3k_dist_stats_workspace_bytes(int64_t m);

/* The five statistics of dist [m] (device) -> out (device double[5]).
 * threshold must not be NaN.  m = 0 writes {0, 0, 0, 0, -inf} (dist and the
 * workspace may be null). */
int s3k_dist_stats(const float* dist, int64_t m, double threshold, double* out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Bytes of the workspace of s3k_sample_mesh for n_faces faces (0 for
 * n_faces <= 0 or n_faces > 2^31 - 2048): areas, cumulative weights, block
 * sums. */
size_t s3k_sample_workspace_bytes(int64_t n_faces);

/* n_samples area-uniform samples of the mesh (definition above).  All
 * pointers but the workspace's are device arrays of the stated shapes;
 * bad and total are written always, points and face only when total > 0. */
int s3k_sample_mesh(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                    int64_t n_samples, uint64_t seed, float* points, int32_t* face, int64_t* bad,
                    int64_t* total, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3K_H */
