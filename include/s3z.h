/*
 * s3z.h — depth loss and depth-metric sums of a batch of rendered depth maps
 * against target depth, forward and backward, in one fused pass each.
 *
 * The reference has no counterpart (it never supervises or scores rendered
 * depth).  The sums are the customary depth-evaluation quantities (abs-rel,
 * sq-rel, RMSE, RMSE-log, delta < 1.25^k), an L1 / L2 data term, and the
 * single-scale gradient-matching term of MiDaS (Ranftl et al. 2020).
 *
 * Inputs per image b, all [B, H, W] float32 contiguous, H, W >= 1:
 *   depth   D = sum z alpha T   (the rasterizer's return_depth output)
 *   alpha   A = sum alpha T
 *   target  z
 *   weight  w, or NULL for 1 (a mask is a 0 / 1 weight)
 *   scale   s_b, device float [B], or NULL for 1
 *
 * Definition.  Everything is in double from the float32 inputs, one rounding
 * per operation (no contraction); every float32 output is rounded once.
 *   a pixel is valid when  z is finite and z > 0,
 *                          D and A are finite, D > 0, A > 0 and A >= alpha_min,
 *                          w is finite and w > 0,
 *                          s_b is finite and s_b > 0
 *   q = D / A,  p = s_b q,  r = p - z;  an invalid pixel has r = 0 and
 *   contributes to nothing
 *   a pair is a valid pixel with its valid right neighbour, or with its valid
 *   lower neighbour; its weight is w_pq = (w_p + w_q) / 2
 * (csrc/depth_loss_math.hpp holds the order of every operation.)
 *
 * Everything is stream-ordered with no host sync; every buffer is the
 * caller's.  No floating-point atomics: the same input gives the same bits,
 * and an image's sums do not depend on B.
 */
#ifndef S3Z_H
#define S3Z_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Index of each per-image sum in `sums` ([B, S3Z_NSUMS] double):
 *   S3Z_SUM_W       sum w
 *   S3Z_SUM_ABS     sum w |r|
 *   S3Z_SUM_SQ      sum w r^2
 *   S3Z_SUM_ABSREL  sum w |r| / z
 *   S3Z_SUM_SQREL   sum w r^2 / z
 *   S3Z_SUM_LOGSQ   sum w (log p - log z)^2
 *   S3Z_SUM_GRAD    sum over pairs w_pq |r_q - r_p|
 *   S3Z_SUM_WG      sum over pairs w_pq
 *   S3Z_SUM_D1..D3  valid pixels with max(p / z, z / p) < 1.25^k, unweighted
 *   S3Z_SUM_N       valid pixels
 *   S3Z_SUM_QZ      sum w q z    (on the unscaled q: the least-squares scale
 *   S3Z_SUM_QQ      sum w q^2     of q onto z is QZ / QQ)
 * S3Z_TILE_W x S3Z_TILE_H is the tile of pixels one workgroup takes. */
enum { S3Z_SUM_W = 0, S3Z_SUM_ABS = 1, S3Z_SUM_SQ = 2, S3Z_SUM_ABSREL = 3, S3Z_SUM_SQREL = 4,
       S3Z_SUM_LOGSQ = 5, S3Z_SUM_GRAD = 6, S3Z_SUM_WG = 7, S3Z_SUM_D1 = 8, S3Z_SUM_D2 = 9,
       S3Z_SUM_D3 = 10, S3Z_SUM_N = 11, S3Z_SUM_QZ = 12, S3Z_SUM_QQ = 13, S3Z_NSUMS = 14,
       S3Z_TILE_W = 64, S3Z_TILE_H = 8 };

/* Bytes of s3z_forward's workspace (the per-workgroup partial sums). */
size_t s3z_workspace_bytes(int B, int H, int W);

/* One pass over the images: every workgroup takes a tile plus the column
 * right of it and the row below it, writes r to rmap ([B, H, W] float32, or
 * NULL) and its S3Z_NSUMS partial sums in a fixed order; a second, tiny
 * launch adds an image's partials in double in a fixed order. */
int s3z_forward(const float* depth, const float* alpha, const float* target,
                const float* weight, const float* scale, int B, int H, int W,
                double alpha_min, float* rmap, double* sums, void* workspace, void* stream);

/* grad_depth, grad_alpha [B, H, W] float32 = dL/dD, dL/dA of
 *   L = sum_b c_abs S3Z_SUM_ABS + c_sq S3Z_SUM_SQ + c_grad S3Z_SUM_GRAD,
 * coef: device float [B, 3] = {c_abs, c_sq, c_grad} per image.  Per valid
 * pixel p, in gather form (each pixel reads its four neighbours),
 *   dL/dr = w (c_abs sign(r) + 2 c_sq r)
 *           + c_grad sum over the pairs containing p of w_pq sign(r_p - r_q),
 *   grad_depth = dL/dr s / A,  grad_alpha = -dL/dr s D / A^2,   sign(0) = 0;
 * both are 0 at invalid pixels.  The scale is a constant of the backward
 * pass, and the other sums have no gradient. */
int s3z_backward(const float* depth, const float* alpha, const float* target,
                 const float* weight, const float* scale, const float* coef,
                 int B, int H, int W, double alpha_min,
                 float* grad_depth, float* grad_alpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3Z_H */
