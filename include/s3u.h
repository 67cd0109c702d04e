/*
 * s3u.h — lens undistortion on the device: cv2.remap(img, mapx, mapy,
 * INTER_LINEAR) with BORDER_CONSTANT 0 on 8-bit frames
 * (splatt3r_slam/dataloader.py:295-296, run on every frame before
 * resize_img when the dataset is calibrated).
 *
 * cv2's 8-bit bilinear remap is integer arithmetic after one quantisation of
 * the map to 1/32 pixel (imgproc/src/remap.cpp, INTER_BITS = 5):
 *     sx = rint(mapx * 32)  (half to even),  ix = clamp(sx >> 5, short range),
 *     fx = sx & 31;  sy, iy, fy likewise;  taps outside the image are 0;
 *     out = ((32-fx)(32-fy) p00 + fx(32-fy) p01 + (32-fx)fy p10 + fx fy p11
 *            + 512) >> 10.
 * The maps are built once per camera on the host
 * (splatt3r_amd/intrinsics.py); the kernel does no floating-point arithmetic
 * beyond the product by 32 and its rounding.
 */
#ifndef S3U_H
#define S3U_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src: [B, H, W, C] uint8 device, C = 1 (greyscale, written to all three
 * output channels) or 3.  mapx/mapy: [out_h, out_w] float32 device, the
 * source coordinates of every output pixel, shared by the B frames.
 * dst: [B, out_h, out_w, 3] uint8 device; must not overlap src.  H and W at
 * most 32767 (ix and iy are clamped to the short range, as cv2's).  Any map
 * value is safe: every tap is bounds-checked.  One launch, stream-ordered, no
 * host sync, no workspace. */
int s3u_remap(const uint8_t* src, int B, int H, int W, int C,
              const float* mapx, const float* mapy, int out_h, int out_w,
              uint8_t* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3U_H */
