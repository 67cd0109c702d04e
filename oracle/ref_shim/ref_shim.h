/*
 * ORACLE — test infrastructure only.  Host shim that lets g++ compile the
 * per-thread kernels cut out of the reference tree by oracle/ref_build.py
 * (refine_matches_kernel / iter_proj_kernel of matching_kernels.cu and the
 * huber .. pose_retr_kernel span of gn_kernels.cu) as plain C++.  Those
 * kernels use no shared memory, no barriers and no warp intrinsics, so one
 * "thread" at a time with blockDim.x = 1 runs them exactly as written.
 *
 * This file holds no reference text: only the few names that text expects.
 */
#ifndef ORACLE_REF_SHIM_H
#define ORACLE_REF_SHIM_H

#include <math.h>
#include <stdint.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>
#include <vector>

#include <c10/util/Half.h>  // the real c10::Half arithmetic (header only)

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline

struct RefDim3 {
  unsigned int x = 0, y = 0, z = 0;
};
/* one thread at a time: the driver sets these before every kernel call */
inline RefDim3 threadIdx, blockIdx, blockDim, gridDim;

namespace torch {

template <typename T>
struct RestrictPtrTraits {
  typedef T* PtrType;
};

/* Stand-in for torch::PackedTensorAccessor32: a pointer plus the trailing
 * sizes / strides; operator[] peels one dimension, the last one yields T&. */
template <typename T, int N, template <typename U> class PtrTraits = RestrictPtrTraits>
struct PackedTensorAccessor32 {
  T* data;
  const int32_t* sizes;
  const int32_t* strides;
  int32_t size(int i) const { return sizes[i]; }
  int32_t stride(int i) const { return strides[i]; }
  PackedTensorAccessor32<T, N - 1, PtrTraits> operator[](int64_t i) const {
    return {data + i * strides[0], sizes + 1, strides + 1};
  }
};

template <typename T, template <typename U> class PtrTraits>
struct PackedTensorAccessor32<T, 1, PtrTraits> {
  T* data;
  const int32_t* sizes;
  const int32_t* strides;
  int32_t size(int i) const { return sizes[i]; }
  int32_t stride(int i) const { return strides[i]; }
  T& operator[](int64_t i) const { return data[i * strides[0]]; }
};

}  // namespace torch

/*
 * cuda::std::numeric_limits.  THE ONE PLACE WHERE THE SHIM DECIDES SEMANTICS.
 * libcu++ specialises numeric_limits for the built-in arithmetic types only;
 * every other type, c10::Half included, gets the primary template, whose
 * min() returns a value-initialised T.  So the initial best score of
 * refine_matches_kernel<c10::Half> (matching_kernels.cu:46) is Half() == +0,
 * not the smallest normal 6.1e-5 that std::numeric_limits<c10::Half>::min()
 * (specialised by c10) would give.  This is the reading DESIGN.md
 * ("refine_matches") and csrc/matching.hip commit to; forwarding c10::Half to
 * std::numeric_limits here changes matches whose best score lies in
 * (0, 6.1e-5] (tests/test_ref_kernels.py, the low-score case).
 */
namespace cuda {
namespace std {

template <typename T, bool kBuiltin = ::std::is_arithmetic<T>::value>
struct numeric_limits {
  static constexpr bool is_specialized = false;
  static T min() { return T(); }
  static T max() { return T(); }
  static T lowest() { return T(); }
};

template <typename T>
struct numeric_limits<T, true> : ::std::numeric_limits<T> {};

}  // namespace std
}  // namespace cuda

/* Contiguous tensor view that owns the size / stride arrays of an accessor. */
template <typename T, int N>
struct RefTensor {
  T* data;
  int32_t sizes[N];
  int32_t strides[N];
  RefTensor(T* p, ::std::initializer_list<int64_t> shape) : data(p) {
    int k = 0;
    for (int64_t s : shape) sizes[k++] = (int32_t)s;
    int32_t st = 1;
    for (int d = N - 1; d >= 0; --d) {
      strides[d] = st;
      st *= sizes[d];
    }
  }
  torch::PackedTensorAccessor32<T, N, torch::RestrictPtrTraits> acc() {
    return {data, sizes, strides};
  }
};

#endif /* ORACLE_REF_SHIM_H */
