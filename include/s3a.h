/*
 * s3a.h — re-anchor the Gaussian map when keyframe poses are re-optimised.
 *
 * The reference has no counterpart: its map (SharedGaussians,
 * splatt3r_slam/frame.py:357-463, here s3w_map) stores kf_id per Gaussian
 * "for provenance" and never reads it, so after the backend rewrites keyframe
 * poses in place (frame.py:269-330) the Gaussians those keyframes contributed
 * stay where the old poses put them.  This pass moves them rigidly (up to
 * scale) with their keyframe: one Sim3 per keyframe applied to the mean and
 * the covariance of every Gaussian that carries its label.
 *
 * Definition (tests/map_reanchor_ref64.py restates it in numpy float64).
 *   pose row   lietorch's [t(3), q(x y z w), s] in float32:
 *              T(x) = s R(q / |q|) x + t.
 *   valid      a row whose 8 entries are finite, with s > 0 and |q| > 0.
 *   anchor     [n_kf, 8] float32, part of the map: row k is the pose of
 *              keyframe k under which the Gaussians labelled k are currently
 *              expressed.  A row with s == 0 is unset; a set row that is not
 *              valid (only a caller can write one) is read as unset.
 *   For each k < n_kf, given poses[k]:
 *     poses[k] invalid            keyframe k is held: no Gaussian moves, the
 *                                 anchor row is kept, *held counts it;
 *     anchor unset, pose valid    anchor[k] = poses[k], nothing moves;
 *     anchor == pose in all eight 32-bit patterns   nothing moves;
 *     otherwise, with M = (s_n / s_o) R_n R_o^T, every row i < *map->n with
 *       kf_id[i] == k gets
 *         mu'    = t_n + M (mu - t_o)
 *         Sigma' = M Sigma M^T
 *       (nothing cancels against |t|), then anchor[k] = poses[k].
 *   Rows with kf_id < 0 (a loaded .ply) or kf_id >= n_kf, and rows at or past
 *   *map->n, are untouched in every field.  Colours, opacities, kf_id and the
 *   count are never written.
 *
 * Arithmetic (csrc/map_reanchor_math.hpp, host + device, built with
 * -ffp-contract=off).  Everything is double on the float32 inputs: the
 * quaternions are normalised in double, R is the usual quadratic form of the
 * unit quaternion, M = (s_n / s_o) (R_n R_o^T) with each entry's three
 * products added left to right, A = M Sigma and Sigma'_ij = sum_l A_il M_jl
 * for i <= j likewise (Sigma the full symmetric matrix of the six stored
 * entries, so the six outputs are those of the symmetric product), and each of
 * the 9 outputs is rounded to float32 once.  A moved row is a pure function of
 * its 9 inputs and the two pose rows: bit-reproducible, independent of n, of
 * the other rows and of the launch geometry; a second call with the same
 * poses finds every anchor equal and moves nothing.
 */
#ifndef S3A_H
#define S3A_H
#include "s3_common.h"
#include "s3w.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace s3a_map_reanchor needs for n_kf keyframes: 16
 * doubles {flag, M[9], t_o[3], t_n[3]} each (0 for n_kf <= 0). */
size_t s3a_reanchor_workspace_bytes(int32_t n_kf);

/* Re-anchor `map` (means and cov_triu of rows i < min(*map->n, map->cap)) from
 * `anchor` to `poses` (both device float [n_kf, 8]) and update `anchor`.
 *   moved, held   optional device int64 counters, written (not added to): the
 *                 rows moved and the keyframes held
 *   workspace     device, 8-byte aligned, >= s3a_reanchor_workspace_bytes(n_kf)
 * means and cov_triu must be 8-byte aligned (16-byte for the staged path).
 * n_kf <= 0 or a workspace that is too small returns S3_ERR_INVALID before
 * any device work.  Two stream-ordered launches (the per-keyframe deltas, then
 * one thread per Gaussian), no host read, no floating-point atomic. */
int s3a_map_reanchor(const s3w_map* map, float* anchor, const float* poses, int32_t n_kf,
                     int64_t* moved, int64_t* held, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Testing and measuring hook: 0 = direct per-lane accesses (the default),
 * 1 = a workgroup with something to move stages its 256 rows through LDS as
 * float4 runs.  Both paths give identical bits. */
void s3a_set_path(int path);

#ifdef __cplusplus
}
#endif
#endif /* S3A_H */
