// rowvec.h -- pieces shared by the kernels in which a thread owns one 16-byte channel vector of [rows][C] activations and a
// workgroup of 256 threads is (1 << lcw) channel vectors x 256 >> lcw runs of rows (mixer.hip, van.hip): vector loads and
// stores, per-channel coefficients, and the ordered sum over a workgroup's runs that makes the partial rows reproducible.
#pragma once
#include "common.h"

namespace htrvt {

constexpr int ROWVEC_NT = 256;

template <typename T>
__device__ __forceinline__ Vec16<T> ld_vec(const T* p, long long elem) {
  using Raw = decltype(Vec16<T>().raw);
  Vec16<T> v;
  v.raw = *reinterpret_cast<const Raw*>(p + elem);
  return v;
}
template <typename T>
__device__ __forceinline__ void st_vec(T* p, long long elem, const Vec16<T>& v) {
  using Raw = decltype(Vec16<T>().raw);
  *reinterpret_cast<Raw*>(p + elem) = v.raw;
}

// CH per-channel float32 coefficients from p + c0 (c0 a multiple of CH), as 16-byte loads where p allows; p == NULL: dflt
template <int CH>
__device__ __forceinline__ void ld_coef(const float* __restrict__ p, int c0, float dflt, float (&o)[CH]) {
  if (p == nullptr) {
#pragma unroll
    for (int e = 0; e < CH; ++e) o[e] = dflt;
  } else if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
      const float4 v = reinterpret_cast<const float4*>(p + c0)[q];
      o[4 * q] = v.x, o[4 * q + 1] = v.y, o[4 * q + 2] = v.z, o[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < CH; ++e) o[e] = p[c0 + e];
  }
}

// sums of v[] over the workgroup's runs (threads of equal cl), in the order of rl; valid in the threads with rl == 0
template <int CH>
__device__ __forceinline__ void run_sum(float (&v)[CH], float* red, int cl, int rl, int lcw) {
  __syncthreads();
#pragma unroll
  for (int e = 0; e < CH; ++e) red[threadIdx.x * CH + e] = v[e];
  __syncthreads();
  if (rl == 0) {
    const int rpb = ROWVEC_NT >> lcw;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      float a = 0.f;
      for (int r = 0; r < rpb; ++r) a += red[((r << lcw) + cl) * CH + e];
      v[e] = a;
    }
  }
}

}  // namespace htrvt
