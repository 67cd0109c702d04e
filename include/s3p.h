/*
 * s3p.h — photometric loss and render-quality sums: masked squared / absolute
 * error and Gaussian-window SSIM of a batch of images, forward and backward.
 *
 * Reference: splatt3r_core/main.py calculate_loss (:199-247, masked MSE) and
 * log_metrics (:249-258, psnr = -10 log10(mse) and a masked SSIM), with
 * utils/compute_ssim.py calling skimage.metrics.structural_similarity(
 * win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) on the
 * host per image.
 *
 * Definition (per channel; x = pred, y = target, both multiplied by the mask
 * first when one is given, the reference's apply_mask):
 *   g[k] = exp(-k^2 / (2 * 1.5^2)), k = -5..5, in double, normalised to sum 1,
 *          rounded to float32;  G = the separable filter with these taps and
 *          scipy's `reflect` border (d c b a | a b c d | d c b a)
 *   ux = G x, uy = G y, uxx = G x^2, uyy = G y^2, uxy = G xy
 *   vx = cn (uxx - ux^2), vy = cn (uyy - uy^2), vxy = cn (uxy - ux uy),
 *          cn = 121/120 with sample_covariance, else 1
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
 *          C1 = 0.01^2, C2 = 0.03^2
 *
 * pred, target: [B, C, H, W] float32 contiguous, C in {1, 3}, H, W >= 11.
 * mask: [B, H, W] float32 of 0 / 1, or NULL.  Everything is stream-ordered
 * with no host sync; every buffer is the caller's.
 */
#ifndef S3P_H
#define S3P_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Index of each per-image sum in `sums` ([B, S3P_NSUMS] double):
 *   S3P_SUM_SQ    sum m (x - y)^2   over channels and pixels
 *   S3P_SUM_ABS   sum m |x - y|
 *   S3P_SUM_MS    sum m S
 *   S3P_SUM_M     sum m             over pixels (H W without a mask)
 *   S3P_SUM_CROP  sum S over the crop [5, H-5) x [5, W-5) (skimage full=False) */
enum { S3P_SUM_SQ = 0, S3P_SUM_ABS = 1, S3P_SUM_MS = 2, S3P_SUM_M = 3, S3P_SUM_CROP = 4,
       S3P_NSUMS = 5 };

/* Bytes of s3p_forward's workspace (the per-workgroup partial sums). */
size_t s3p_workspace_bytes(int B, int C, int H, int W);

/* Bytes of s3p_forward's `derivs` (three [B, C, H, W] float32 maps). */
size_t s3p_derivs_bytes(int B, int C, int H, int W);

/* One pass over the images: every workgroup takes a tile plus a 5-pixel halo
 * into LDS, filters the five moment maps (rows, then columns), computes S and
 * writes its partial sums in a fixed order; a second, tiny launch adds the
 * partials in double in a fixed order.  No floating-point atomics: the same
 * input gives the same bits.
 * smap: [B, C, H, W] or NULL.  derivs: dS/dux, dS/duxx, dS/duxy per pixel
 * (what s3p_backward reads), or NULL when no backward follows. */
int s3p_forward(const float* pred, const float* target, const float* mask,
                int B, int C, int H, int W, int sample_covariance,
                float* smap, float* derivs, double* sums, void* workspace, void* stream);

/* grad [B, C, H, W] = dL/dpred
 *   = m ( Gt[w dS/dux] + 2x Gt[w dS/duxx] + y Gt[w dS/duxy]
 *         + 2 a (x - y) + b sign(x - y) ),          sign(0) = 0,
 * Gt the adjoint of the reflect-padded filter.  The weight of S at a pixel is
 *   w = wmap (when given) + c_ms m + c_crop [pixel inside the crop];
 * coef: device float [B, 4] = {a, b, c_ms, c_crop} per image, i.e. dL/d of the
 * sums S3P_SUM_SQ, _ABS, _MS, _CROP; wmap: [B, C, H, W] = dL/dS, or NULL.
 * derivs: as written by s3p_forward for the same pred, target, mask. */
int s3p_backward(const float* pred, const float* target, const float* mask,
                 const float* derivs, const float* wmap, const float* coef,
                 int B, int C, int H, int W, float* grad, void* stream);

/* The 11 float32 filter taps g[-5..5]. */
void s3p_window(float* taps);

#ifdef __cplusplus
}
#endif
#endif /* S3P_H */
