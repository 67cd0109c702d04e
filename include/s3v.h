/*
 * s3v.h — map compaction: Gaussians whose centres fall in the same voxel are
 * replaced by their moment-matched merge.
 *
 * The reference has no counterpart: its map buffer (SharedGaussians,
 * splatt3r_slam/frame.py:357-463, here s3w_map_append) throws the oldest half
 * away when it is full, although neighbouring keyframes each predict a full
 * set of Gaussians for the surfaces they share.  This pass removes those
 * duplicates instead.
 *
 * Definition (tests/map_compact_ref64.py restates it in numpy float64):
 *   key      per axis i = floor(((double)x - origin) / voxel) + 2^20, clamped
 *            to [0, 2^21 - 1]; key = ix << 42 | iy << 21 | iz (63 bits).
 *            Double subtraction, division and floor are correctly rounded, so
 *            numpy float64 gives the same integers.  The clamp folds
 *            everything further than 2^20 voxels from the origin (10 km at
 *            1 cm voxels) into the outermost voxel of that side.
 *   dropped  a row with a non-finite mean, covariance entry, colour or
 *            opacity belongs to no group: it is counted in *dropped and its
 *            `group` entry is -1.
 *   group    all kept rows with one key.
 *   weights  w_i = opacity_i; if a group's weights sum to exactly 0, every
 *            w_i = 1.  W = sum w_i.
 *   mean     mu = sum w_i mu_i / W
 *   cov      Sigma = sum w_i (Sigma_i + (mu_i - mu)(mu_i - mu)^T) / W
 *   colour   sum w_i c_i / W
 *   opacity  sum w_i o_i / W: k copies of one surface are each a complete
 *            description of it, so the merge does not stack them.
 *   kf_id    that of the group's lowest-index member.
 *   order    output rows are ordered by `first`, the lowest input index of
 *            each group: a map that was oldest-first stays so, and kf_id stays
 *            non-decreasing where it was.
 *   A group of one is copied through bit for bit, all five fields.
 *
 * Arithmetic.  Every sum is double and is taken in an order the input alone
 * fixes: a group's members in (key, input index) order, cut into chunks of 64
 * counted from the group's first member; a chunk is summed front to back, a
 * group of more than one chunk then has its chunk sums added by one workgroup
 * of 256 threads (thread t takes chunks t, t + 256, ... in order, then a
 * butterfly over each wave's lanes, then the four waves in order).  None of
 * this depends on the launch geometry, and there is no floating-point atomic:
 * two calls give the same bits.  Positions are accumulated as offsets from the
 * group's first member d_i = mu_i - mu_first (so nothing cancels against
 * |mu|^2; what cancels in sum w d d^T / W - dbar dbar^T is bounded by the
 * voxel), and each output is rounded to float32 once.
 *
 * A merged mean is a convex combination of its members and the key is
 * monotone in x, so it stays in its voxel: a second call with the same origin
 * and voxel finds only singletons and returns every field bit for bit.
 */
#ifndef S3V_H
#define S3V_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const float* means;      /* [n_max, 3] */
  const float* cov_triu;   /* [n_max, 6] xx xy xz yy yz zz */
  const float* colors;     /* [n_max, 3] */
  const float* opacities;  /* [n_max]    */
  const int32_t* kf_id;    /* [n_max]    */
} s3v_in;

typedef struct {
  float* means;
  float* cov_triu;
  float* colors;
  float* opacities;
  int32_t* kf_id;
} s3v_out;

/* Bytes of the workspace s3v_merge needs for n_max rows (0 for n_max <= 0). */
size_t s3v_merge_workspace_bytes(int64_t n_max);

/* Merge rows i < n = min(*n_dev, n_max) (n_dev device int64, NULL: n_max) of
 * `in` into the first *m rows of `out`:
 *   origin  host double[3], finite;  voxel > 0 and finite
 *   first   device int64 [n_max]: first[r], r < *m, the lowest input index of
 *           output row r's group
 *   group   device int64 [n_max]: group[i], i < n, the output row input row i
 *           went to, or -1 for a dropped row
 *   m, dropped  device int64 counters, written (not added to)
 * Entries of the outputs at and past *m (group: n) are left untouched.  Every
 * buffer is the caller's; the outputs must not overlap the inputs.
 * workspace: device, 256-byte aligned, >= s3v_merge_workspace_bytes(n_max).
 * The passes: keys and the occupied cell range; a stable 64-bit LSD radix sort
 * of (key, index) on the keys packed to that range (order kept), in as many
 * 8-bit passes as the packed keys have digits, at most eight; group heads; two
 * scans (each row's group start; the output row of each head in input order);
 * the chunked sums; the long groups.
 * n_max < 2^31 - 2048.  Stream-ordered, no host read. */
int s3v_merge(const s3v_in* in, const int64_t* n_dev, int64_t n_max, const double* origin,
              double voxel, const s3v_out* out, int64_t* first, int64_t* group, int64_t* m,
              int64_t* dropped, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3V_H */
