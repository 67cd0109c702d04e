/*
 * s3c.h — co-visibility loss mask: which pixels of a set of target views have
 * a directly corresponding pixel in any view of a set of context views.
 *
 * Reference: splatt3r_core/utils/loss_mask.py calculate_in_frustum_mask (with
 * the projections of utils/geometry.py), run by training_step,
 * validation_step and test_step of splatt3r_core/main.py before every
 * calculate_loss; about 40 elementwise / einsum launches, b v1 v2 grid_sample
 * calls and two batched inverses there, two launches here.
 *
 * Definition, per target pixel (b, i, y, x) with d = depth_1[b, i, y, x], all
 * in float32 with every product and sum rounded on its own (no contraction),
 * sums running left to right:
 *   cam   = (inverse(K_1[b, i]) (x, y, 1)) d        x, y the integer pixel
 *                                                   indices, no half-pixel offset
 *   world = c2w_1[b, i] (cam, 1)
 * and per context view j:
 *   cp    = inverse(c2w_2[b, j]) (world, 1)         rows 0..2
 *   z     = cp.z
 *   (u, v) = (K_2[b, j] (cp / cp.z)).xy
 *   fr_j  = u > 0 && u < W && v > 0 && v < H
 *   s_j   = bilinear sample of depth_2[b, j] at (u - 0.5, v - 0.5); taps
 *           outside the image contribute 0 (grid_sample, align_corners=False,
 *           padding_mode='zeros')
 *   md_j  = z == s_j || |z - s_j| <= 0.1 + 1e-5 |s_j|      (torch.isclose,
 *           atol 1e-1, default rtol)
 *   mask  = (any_j fr_j) && (d > 1e-6) && (any_j md_j)
 * The two `any` run separately over the context views, and there is no z > 0
 * test: both are the reference's behaviour and part of the contract.  Every
 * comparison with a NaN is false; a non-finite or huge (u, v) reads no memory
 * (each tap is bound-checked in floating point before it becomes an index).
 *
 * The inverses are computed once per view by a one-thread-per-view prologue
 * kernel, in closed form (adjugate / cofactors) in double, rounded to float32
 * into the workspace.  They are general: K may carry skew, c2w a Sim3 scale
 * (s R | t).  A singular matrix gives non-finite entries and hence a false
 * mask (the reference raises there).
 */
#ifndef S3C_H
#define S3C_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bits of `conditions`. */
enum { S3C_COND_FRUSTUM = 1, S3C_COND_DEPTH = 2, S3C_COND_MATCH = 4 };

/* Bytes of s3c_loss_mask's workspace (the float32 inverses of every K_1 and
 * every c2w_2). */
size_t s3c_loss_mask_workspace_bytes(int B, int V1, int V2);

/* depth_1 [B,V1,H,W], K_1 [B,V1,9], c2w_1 [B,V1,16]; depth_2 [B,V2,H,W], K_2 [B,V2,9],
 * c2w_2 [B,V2,16]; all float32, row-major, device.  mask [B,V1,H,W] uint8 (0/1; the storage
 * of a torch.bool); mask_f32 same shape or NULL; conditions same shape uint8 or NULL
 * (S3C_COND_FRUSTUM = any fr, S3C_COND_DEPTH = d > 1e-6, S3C_COND_MATCH = any md).
 * Two launches on `stream`, no host sync, no library call. */
int s3c_loss_mask(const float* depth_1, const float* K_1, const float* c2w_1,
                  const float* depth_2, const float* K_2, const float* c2w_2,
                  int B, int V1, int V2, int H, int W,
                  uint8_t* mask, float* mask_f32, uint8_t* conditions,
                  void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3C_H */
