/*
 * s3o.h — optimiser over the Gaussian map's splat parameters: the activation
 * that turns parameter rows into rasterizer inputs, and the fused chain rule
 * + Adam step that consumes the rasterizer's gradients.
 *
 * The reference trains network weights, never Gaussians; the semantics here
 * are the INRIA 3DGS parametrisation (the project's .ply, include/s3w.h) and
 * torch.optim.Adam without weight decay or amsgrad.
 *
 * A parameter row is the 14-float rows14 layout of s3w_map_from_splats:
 *   x y z, f_dc_0..2, logit opacity, log scale_0..2, rot w x y z (raw, not
 *   necessarily unit).
 * Five parameter groups, each with its own learning rate: means, f_dc,
 * opacity, scale, rotation.
 */
#ifndef S3O_H
#define S3O_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  float lr[5];        /* means, f_dc, opacity, scale, rotation */
  float beta1, beta2; /* in [0, 1) */
  float eps;          /* > 0 */
  float bias1;        /* 1 - beta1^t, computed by the host in double */
  float bias2_sqrt;   /* sqrt(1 - beta2^t), likewise */
  float render_scale; /* the scale-invariant factor 1 / near, > 0 */
} s3o_adam;

/* rows14 [n, 14] -> the five tensors GaussianRasterizer takes, with the
 * scale-invariant factor s = render_scale applied:
 *   means3D [n, 3]     s xyz
 *   shs [n, 1, 3]      f_dc (the rasterizer's sh_degree 0 path computes
 *                      max(0, C0 sh + 0.5) and its backward carries the clamp)
 *   opacities [n, 1]   sigmoid(logit)
 *   scales [n, 3]      s exp(log scale)
 *   rotations [n, 4]   q / |q| in (r, x, y, z) order; a zero quaternion is
 *                      the identity
 * opacities, scales and rotations are formed in double and rounded once: each
 * is the float32 nearest the exact value.
 * rows14 must be 8-byte and rotations 16-byte aligned.  n == 0 returns S3_OK
 * without a launch.  Stream-ordered, no host sync. */
int s3o_activate(const float* rows14, int64_t n, float render_scale, float* means3D, float* shs,
                 float* opacities, float* scales, float* rotations, void* stream);

/* One fused step: the chain rule from the rasterizer's gradients of the five
 * activated tensors (layouts as above) to the row,
 *   g_xyz = s dmeans3D, g_fdc = dsh, g_logit = dop o (1 - o),
 *   g_logscale = dscales scales, g_q = (dr - qh (qh . dr)) / |q| (zero for a
 *   zero quaternion),
 * the activations recomputed from the row, then Adam:
 *   m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g^2,
 *   p -= (lr / bias1) m / (sqrt(v) / bias2_sqrt + eps)
 * on rows14, exp_avg and exp_avg_sq ([n, 14] each) in place.
 * radii (int32 [n], the rasterizer's output) or NULL: a row with
 * radii[i] <= 0 is left untouched, and so are its two moment rows (nothing
 * but radii[i] is loaded, nothing stored): 3DGS's sparse Adam.  NULL: dense.
 * A row whose 14 incoming gradients hold a NaN or an Inf is left untouched
 * too and counted in *skipped (device int32, added to; or NULL).
 * One thread per Gaussian: a row's result is a pure function of its own
 * inputs, bit-reproducible and independent of n and of its position.
 * rows14, exp_avg and exp_avg_sq must be 8-byte, d_rotations 16-byte
 * aligned.  n == 0 returns S3_OK without a launch.  Stream-ordered, no host
 * sync. */
int s3o_adam_step(float* rows14, float* exp_avg, float* exp_avg_sq, int64_t n,
                  const float* d_means3D, const float* d_shs, const float* d_opacities,
                  const float* d_scales, const float* d_rotations, const int32_t* radii,
                  const s3o_adam* hp, int32_t* skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3O_H */
