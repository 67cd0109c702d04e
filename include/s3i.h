/*
 * s3i.h — device-side frame ingest: raw uint8 HxWx3 frames -> the network's
 * input, bit for bit what the host path (splatt3r_utils.resize_img:
 * PIL.Image.resize LANCZOS/BICUBIC + centre crop + ImgNorm,
 * splatt3r_slam/splatt3r_utils.py:646-693) produces.
 *
 * Pillow's 8-bit resample is fixed-point integer arithmetic
 * (libImaging/Resample.c): per axis a table of int32 coefficients scaled by
 * 2^22 (`coeffs` [out, ksize]) and of source windows (`bounds` [out, 2] =
 * {xmin, count}); a horizontal pass into a uint8 image, then a vertical pass
 * over that image, each sample
 *     out = clamp((2^21 + sum_k pix[xmin + k] * coeffs[k]) >> 22, 0, 255)
 * with int32 accumulation and an arithmetic shift.  The tables are built on
 * the host (splatt3r_amd/ingest.py resample_tables); the kernels here do no
 * floating-point arithmetic: ImgNorm is a 256-entry table lookup.
 */
#ifndef S3I_H
#define S3I_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src: [B, in_h, in_w, 3] uint8 device.  hk/hb: horizontal coefficients
 * [res_w, h_ksize] and bounds [res_w, 2] (device int32), or hk == NULL for
 * no horizontal pass (then res_w must equal in_w); vk/vb likewise for the
 * vertical pass to res_h rows.  Only the window [crop_y0, crop_y0 + crop_h)
 * x [crop_x0, crop_x0 + crop_w) of the resized image is computed.
 * norm_lut: device float[256], the normalised value of every byte.
 * img: [B, 3, crop_h, crop_w] float32, uimg: [B, crop_h, crop_w, 3] uint8 or
 * NULL.  workspace: s3i_workspace_bytes() bytes when s3i_fused_fits() is 0
 * (or the two-launch path is forced), else unused and may be NULL.
 * Stream-ordered, no host sync. */
int s3i_ingest(const uint8_t* src, int B, int in_h, int in_w,
               const int32_t* hk, const int32_t* hb, int h_ksize, int res_w,
               const int32_t* vk, const int32_t* vb, int v_ksize, int res_h,
               int crop_x0, int crop_y0, int crop_w, int crop_h,
               const float* norm_lut, float* img, uint8_t* uimg,
               void* workspace, void* stream);

/* Bytes of the uint8 intermediate of the two-launch path. */
size_t s3i_workspace_bytes(int B, int in_h, int res_w);

/* 1 when one launch does both passes out of LDS (a tile's source span,
 * intermediate and coefficients fit a workgroup's 64 KiB), 0 when the
 * intermediate goes through `workspace` in two launches.  A ksize of 0
 * stands for "no pass on that axis". */
int s3i_fused_fits(int in_h, int in_w, int h_ksize, int res_w, int v_ksize, int res_h);

/* Testing hook: 0 = automatic, 1 = always the two-launch path.  Both paths
 * give identical results. */
void s3i_set_path(int path);

#ifdef __cplusplus
}
#endif
#endif /* S3I_H */
