/*
 * s3x.h — photometric refinement of camera poses: the gradient of a render
 * loss with respect to the camera pose, reduced from the per-Gaussian
 * gradients gsr_backward writes, and the Adam step on the pose.
 *
 * The reference has no counterpart.  The rasterizer's forward depends on the
 * camera and the Gaussians only through view-space quantities (SH degree 0 or
 * colors_precomp; with SH degree > 0 the view direction breaks this), so
 * moving the camera by a rigid motion in its own frame is moving every
 * Gaussian by the inverse motion, and dL/dpose is a sum over the Gaussians of
 * gradients the backward already has.  The backward's three conventions (the
 * Jacobian clamp constant, straight-through 0.99, no gradient through order
 * and radius) carry over unchanged.
 *
 * The pose is camera-to-world, T_WC = (s R | t), and moves as
 *   T_WC <- T_WC Exp(xi),  xi = (rho, phi):
 * the twist is in the camera's own frame.  The rotation optimiser's rates are
 * MonoGS's.
 */
#ifndef S3X_H
#define S3X_H
#include "s3_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace s3x_pose_grad needs for n rows (0 for n < 0). */
size_t s3x_pose_grad_workspace_bytes(int64_t n);

/* out[6] (device, double) = dL/dxi at xi = 0, in view-space units:
 *   viewmatrix [16]  the rasterizer's device view matrix (float32, row-vector
 *                    convention, p_view = [p 1] vm); A = vm[:3,:3]^T,
 *                    b = vm[3,:3].  A may be a scaled rotation: A^-T is
 *                    formed, not assumed equal to A.
 *   means3D, d_means3D [n, 3]
 *   either cov3D, d_cov3D [n, 6] (xx xy xz yy yz zz; the gradient's
 *   off-diagonal entries are those of the 6-vector, i.e. twice the symmetric
 *   matrix gradient's) or rotations, d_rotations [n, 4] (r, x, y, z), the
 *   other pair NULL.  Rotations must be unit, as s3o_activate writes them:
 *   the quaternion form below is the derivative only on the unit sphere.
 *   radii int32 [n] (the rasterizer's) or NULL: a row with radii[i] <= 0
 *   contributes nothing and nothing else of it is loaded.  NULL: dense.
 * With t_i = A mu_i + b and g_i = A^-T dL/dmu_i:
 *   dL/drho = - sum g_i,   dL/dphi = - sum (t_i x g_i + c_i)
 *   covariance form: c_i = 2 axial(G_v S_v - S_v G_v), S_v = A S A^T,
 *     G_v = A^-T G A^-1, axial(X) = (X_21, X_02, X_10)
 *   rotation form:   c_i = R_c w_i, R_c = A / cbrt(det A) the rotation of A,
 *     w_i = 1/2 (q_r dq_v - dq_r q_v + q_v x dq_v)
 * A row with a non-finite input among those it loads contributes nothing and
 * is counted in *skipped (device int32, added to; or NULL).
 * Per-row arithmetic and every sum are double.  The order of the sums is
 * fixed (in a wave, across a workgroup's waves, one partial per workgroup in
 * the workspace, a second launch of one workgroup over the partials in index
 * order) and there is no floating-point atomic: out is a pure function of the
 * inputs and n, bit for bit.  n == 0 or every row culled: six exact zeros.
 * workspace: device, 8-byte aligned, >= s3x_pose_grad_workspace_bytes(n).
 * rotations and d_rotations must be 16-byte aligned.  Stream-ordered, no host
 * read. */
int s3x_pose_grad(const float* viewmatrix, const float* means3D, const float* d_means3D,
                  const float* cov3D, const float* d_cov3D, const float* rotations,
                  const float* d_rotations, const int32_t* radii, int64_t n, double* out,
                  int32_t* skipped, void* workspace, size_t workspace_bytes, void* stream);

typedef struct {
  double lr_translation; /* >= 0, on rho (caller's units) */
  double lr_rotation;    /* >= 0, on phi */
  double beta1, beta2;   /* in [0, 1) */
  double eps;            /* > 0 */
  double bias1;          /* 1 - beta1^t */
  double bias2_sqrt;     /* sqrt(1 - beta2^t) */
  double render_scale;   /* the scale-invariant factor 1 / near, > 0 */
} s3x_pose_adam;

/* One view's step, one launch of one thread, everything in double:
 *   g = (render_scale grad[0..2], grad[3..5])   (s3x_pose_grad's output is in
 *       view-space units, the pose in the caller's: rho' = rho / render_scale)
 *   Adam (torch.optim.Adam without weight decay or amsgrad) on the six twist
 *   components with moments exp_avg, exp_avg_sq [6]:
 *       m = m + (1 - beta1) (g - m),  v = beta2 v + (1 - beta2) g^2,
 *       delta = (lr / bias1) m / (sqrt(v) / bias2_sqrt + eps)
 *   T_WC <- T_WC Exp(-delta)      (T_WC [16] row-major; SE(3) Exp with series
 *       near zero; a uniform scale of the 3 x 3 block is preserved)
 * and then that view's float32 camera from the new pose, as s3r_camera and
 * render.camera_settings form it:
 *   ext = T_WC with ext[:3,3] *= render_scale
 *   viewmatrix = (ext^-1)^T, projmatrix = viewmatrix @ proj_t, campos = ext[:3,3]
 * proj_t [16]: the transposed projection matrix (float32, row-major, device).
 * A gradient with a NaN or an Inf leaves the pose and both moments untouched
 * (the camera is still written, from the unchanged pose).  grad NULL: no step,
 * the camera only; exp_avg and exp_avg_sq may then be NULL.
 * All pointers device.  Stream-ordered, no host read. */
int s3x_pose_step(double* T_WC, double* exp_avg, double* exp_avg_sq, const double* grad,
                  const s3x_pose_adam* hp, const float* proj_t, float* viewmatrix,
                  float* projmatrix, float* campos, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3X_H */
