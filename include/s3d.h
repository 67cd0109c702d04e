/*
 * s3d.h — adaptive density control of the Gaussian map's splat parameters:
 * the per-Gaussian statistics of the refinement steps, the pass that prunes,
 * clones and splits rows (with their Adam moments), and the opacity reset.
 *
 * The reference trains network weights, never Gaussians; the semantics are
 * INRIA 3DGS's densify_and_prune / reset_opacity restated as one decision
 * per row, so the result is a pure function of the inputs and the output
 * order is fixed.  Two differences from INRIA: the prune tests are made on
 * the parent before growth (INRIA tests the children afterwards), and a row
 * with a non-finite entry is pruned.
 *
 * A parameter row is the 14-float rows14 layout of s3o.h:
 *   x y z, f_dc_0..2, logit opacity, log scale_0..2, rot w x y z (raw).
 */
#ifndef S3D_H
#define S3D_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  float grad_threshold;      /* grow when grad_accum / denom >= this */
  float split_scale;         /* a growing row splits when max exp(log scale) > this */
  float min_opacity;         /* prune when sigmoid(logit) < this */
  float max_scale;           /* > 0: prune when max exp(log scale) > this (world units) */
  int32_t max_screen_radius; /* > 0: prune when max_radii > this (pixels) */
  uint64_t seed;             /* Philox key */
  uint32_t pass;             /* Philox counter word 2: the index of this pass */
} s3d_params;

/* Statistics of one refinement step.  d_means2D [n, 3]: the rasterizer
 * backward's dL_dmeans2D (INRIA's NDC convention; only x and y are read),
 * radii [n]: the same forward's int32 radii.  For a row with radii > 0:
 *   grad_accum += sqrt(dx^2 + dy^2), denom += 1,
 *   max_radii = max(max_radii, radii).
 * For a row with radii <= 0 only radii[i] is loaded and nothing is stored; a
 * row with a non-finite dx or dy is left untouched.  grad_accum float32 [n],
 * denom and max_radii int32 [n], in place.  n == 0 returns S3_OK without a
 * launch.  Stream-ordered, no host sync. */
int s3d_accumulate(const float* d_means2D, const int32_t* radii, int64_t n, float* grad_accum,
                   int32_t* denom, int32_t* max_radii, void* stream);

/* Bytes of workspace s3d_densify needs for n input rows (one decision code
 * per row and two counts per block of 256 rows). */
size_t s3d_workspace_bytes(int64_t n);

/* One density pass over n rows and their two Adam moment rows ([n, 14] each).
 *
 * Decision, per row, in this order, with o = sigmoid(logit) and
 * s_k = exp(log scale_k) as s3o_activate forms them (in double, rounded
 * once; world units), smax = max s_k and avg = denom > 0 ? grad_accum /
 * denom : 0:
 *   prune  any of the 14 entries non-finite; o < min_opacity;
 *          max_scale > 0 && smax > max_scale;
 *          max_screen_radius > 0 && max_radii > max_screen_radius
 *   grow   otherwise, when avg >= grad_threshold: split if
 *          smax > split_scale, else clone
 *   keep   otherwise
 *
 * Capacity: with B the number of rows not pruned (B <= n <= cap), every
 * growing row asks for one extra row, and row i's is granted iff the number
 * of growing rows before i is < cap - B; a denied row is kept as it is.
 * n_out = B + min(growing rows, cap - B) <= cap.
 *
 * Output rows keep input order, a row's outputs adjacent:
 *   keep   the row and its two moment rows, bit for bit
 *   clone  the original with its moments, then a bit-identical copy with
 *          zero moments
 *   split  children k = 0, 1 in the parent's place, zero moments:
 *          mean_k = mu + R (s * eps_k) in float32, R of q / |q| (a zero
 *          quaternion is the identity); log scale -= float32(log 1.6); f_dc,
 *          the logit and the raw quaternion copied bit for bit.  eps_k:
 *          Philox4x32-10, counter (i lo32, i hi32, pass, k), key (seed lo32,
 *          seed hi32); words x_j -> u_j = (x_j + 0.5) / 2^32; Box-Muller in
 *          double on (u0, u1) and (u2, u3), each normal rounded to float32
 *          once, the first three used.
 * origin [n_out] int32: i for a kept row or a clone's original, ~i for a
 * clone's copy or a split child.
 * n_out: device int64.  counts: device int32[4] = pruned, cloned, split
 * (granted ones), denied.
 *
 * Outputs (out_rows, out_exp_avg, out_exp_avg_sq [cap, 14], origin [cap])
 * must not overlap the inputs.  Row arrays 8-byte aligned, workspace 4-byte.
 * n < 0, cap < n, n >= 2^31, a null pointer, a short workspace: an error
 * before any device work.  n == 0 returns S3_OK without a launch (n_out and
 * counts are then not written).  Three launches (classify + block counts,
 * scan of the block counts, emit), stream-ordered, no host sync: the emit
 * reads the totals the scan wrote.  A row's outputs are a pure function of
 * its inputs, its index, seed and pass. */
int s3d_densify(const float* rows14, const float* exp_avg, const float* exp_avg_sq, int64_t n,
                const float* grad_accum, const int32_t* denom, const int32_t* max_radii,
                const s3d_params* params, int64_t cap, float* out_rows, float* out_exp_avg,
                float* out_exp_avg_sq, int32_t* origin, int64_t* n_out, int32_t* counts,
                void* workspace, size_t workspace_bytes, void* stream);

/* 3DGS's opacity reset: logit = min(logit, logit_cap) and the opacity column
 * of both moment arrays zeroed, for every row; nothing else is touched.
 * logit_cap: the host computes logit(0.01) in double and rounds it once.
 * n == 0 returns S3_OK without a launch.  Stream-ordered, no host sync. */
int s3d_reset_opacity(float* rows14, float* exp_avg, float* exp_avg_sq, int64_t n,
                      float logit_cap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3D_H */
