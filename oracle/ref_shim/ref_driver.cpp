/*
 * ORACLE — test infrastructure only.  extern "C" entry points over raw
 * pointers for the reference's per-thread kernels.  The kernel text itself is
 * not here: oracle/ref_build.py cuts it out of the reference tree into
 * oracle/_ref/ref_matching_cut.inc and oracle/_ref/ref_gn_cut.inc at build
 * time (neither is committed) and this file includes the two cuts.
 *
 * Every kernel runs one "thread" at a time: blockDim.x = 1, threadIdx.x = 0,
 * blockIdx.x = query index, blockIdx.y = batch index, which is what the
 * reference's launchers (matching_kernels.cu:83-115, :278-315) amount to for
 * kernels without any cross-thread communication.
 */
#include "ref_shim.h"

namespace ref_matching {
#include "ref_matching_cut.inc"
}  // namespace ref_matching

namespace ref_gn {
#include "ref_gn_cut.inc"
}  // namespace ref_gn

namespace {

void one_thread(unsigned bx, unsigned by) {
  blockDim = RefDim3{1, 1, 1};
  threadIdx = RefDim3{0, 0, 0};
  blockIdx = RefDim3{bx, by, 0};
}

template <typename scalar_t>
void refine_matches(const void* D11, const void* D21, const int64_t* p1, int64_t* p1_new, int b,
                    int h, int w, int n, int f, int radius, int dilation_max) {
  static_assert(sizeof(long) == sizeof(int64_t), "the kernels index p1 as long");
  RefTensor<scalar_t, 4> d11((scalar_t*)D11, {b, h, w, f});
  RefTensor<scalar_t, 3> d21((scalar_t*)D21, {b, n, f});
  RefTensor<long, 3> p((long*)p1, {b, n, 2});
  RefTensor<long, 3> pn((long*)p1_new, {b, n, 2});
  for (int bi = 0; bi < b; ++bi)
    for (int i = 0; i < n; ++i) {
      one_thread((unsigned)i, (unsigned)bi);
      ref_matching::refine_matches_kernel<scalar_t>(d11.acc(), d21.acc(), p.acc(), pn.acc(),
                                                    radius, dilation_max);
    }
}

}  // namespace

extern "C" {

/* D11 [b,h,w,f], D21 [b,n,f] as IEEE fp16 bit patterns (c10::Half) */
void ref_refine_matches_half(const uint16_t* D11, const uint16_t* D21, const int64_t* p1,
                             int64_t* p1_new, int b, int h, int w, int n, int f, int radius,
                             int dilation_max) {
  static_assert(sizeof(c10::Half) == 2, "c10::Half is its bit pattern");
  refine_matches<c10::Half>(D11, D21, p1, p1_new, b, h, w, n, f, radius, dilation_max);
}

void ref_refine_matches_float(const float* D11, const float* D21, const int64_t* p1,
                              int64_t* p1_new, int b, int h, int w, int n, int f, int radius,
                              int dilation_max) {
  refine_matches<float>(D11, D21, p1, p1_new, b, h, w, n, f, radius, dilation_max);
}

/* p_new and converged must come in zeroed, as the reference launcher
 * allocates them (max_iter = 0 never writes converged). */
void ref_iter_proj(const float* rays, const float* pts, const float* p_init, float* p_new,
                   uint8_t* converged, int b, int h, int w, int n, int max_iter,
                   float lambda_init, float cost_thresh) {
  static_assert(sizeof(bool) == 1, "converged is one byte per point");
  RefTensor<float, 4> r((float*)rays, {b, h, w, 9});
  RefTensor<float, 3> p3((float*)pts, {b, n, 3});
  RefTensor<float, 3> pi((float*)p_init, {b, n, 2});
  RefTensor<float, 3> pn(p_new, {b, n, 2});
  RefTensor<bool, 2> cv((bool*)converged, {b, n});
  for (int bi = 0; bi < b; ++bi)
    for (int i = 0; i < n; ++i) {
      one_thread((unsigned)i, (unsigned)bi);
      ref_matching::iter_proj_kernel(r.acc(), p3.acc(), pi.acc(), pn.acc(), cv.acc(), max_iter,
                                     lambda_init, cost_thresh);
    }
}

/* poses [num_poses,8] in place, dx [num_poses-num_fix,7] */
void ref_pose_retr(float* poses, const float* dx, int64_t num_poses, int64_t num_fix) {
  RefTensor<float, 2> P(poses, {num_poses, 8});
  RefTensor<float, 2> D((float*)dx, {num_poses - num_fix, 7});
  one_thread(0, 0);
  ref_gn::pose_retr_kernel(P.acc(), D.acc(), (int)num_fix);
}

/* Sim3 element = t(3) q(xyzw) s(1); tangent = tau(3) phi(3) sigma */
void ref_sim3_exp_batch(const float* xi, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    float* o = out + i * 8;
    ref_gn::expSim3(xi + i * 7, o, o + 3, o + 7);
  }
}

void ref_sim3_retr_batch(const float* T, const float* xi, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const float* a = T + i * 8;
    float* o = out + i * 8;
    ref_gn::retrSim3(xi + i * 7, a, a + 3, a + 7, o, o + 3, o + 7);
  }
}

void ref_sim3_act_batch(const float* T, int64_t nT, const float* X, float* Y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const float* a = T + (nT == 1 ? 0 : i) * 8;
    ref_gn::actSim3(a, a + 3, a + 7, X + i * 3, Y + i * 3);
  }
}

/* a * b from the reference's parts: t = actSim3(a, t_b), q = quat_comp(q_a,
 * q_b) (NOT re-normalised: the reference has no group product of its own,
 * the normalisation is lietorch's and is applied by the caller), s = s_a s_b */
void ref_sim3_mul_batch(const float* A, const float* B, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const float *a = A + i * 8, *b = B + i * 8;
    float* o = out + i * 8;
    ref_gn::actSim3(a, a + 3, a + 7, b, o);
    ref_gn::quat_comp(a + 3, b + 3, o + 3);
    o[7] = a[7] * b[7];
  }
}

/* Ti^-1 * Tj */
void ref_sim3_rel_batch(const float* Ti, const float* Tj, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const float *a = Ti + i * 8, *b = Tj + i * 8;
    float* o = out + i * 8;
    ref_gn::relSim3(a, a + 3, a + 7, b, b + 3, b + 7, o, o + 3, o + 7);
  }
}

void ref_sim3_adj_inv_batch(const float* T, const float* X, float* Y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const float* a = T + i * 8;
    ref_gn::apply_Sim3_adj_inv(a, a + 3, a + 7, X + i * 7, Y + i * 7);
  }
}

void ref_huber_batch(const float* r, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = ref_gn::huber(r[i]);
}

}  // extern "C"
