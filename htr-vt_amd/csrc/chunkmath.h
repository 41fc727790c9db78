// chunkmath.h -- arithmetic on 16-byte chunks of a head slice as they are stored, shared by the window attention kernels
// that keep scores on the VALU (lgp.hip, swin.hip): a dot product of two chunks and a two-row accumulation.
#pragma once
#include "common.h"

namespace htrvt {

// acc + dot product of two 16-byte chunks.  bfloat16: v_dot2c_f32_bf16 takes the packed pairs as they are stored, so the
// score products cost one instruction per two elements and no conversion
template <typename T>
struct ChunkDot;
template <>
struct ChunkDot<float> {
  static __device__ __forceinline__ float run(float acc, const float4& a, const float4& b) {
    acc += a.x * b.x;
    acc += a.y * b.y;
    acc += a.z * b.z;
    acc += a.w * b.w;
    return acc;
  }
};
template <>
struct ChunkDot<bf16_t> {
  static __device__ __forceinline__ float run(float acc, const uint4& a, const uint4& b) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.x), __builtin_bit_cast(bf16x2_t, b.x), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.y), __builtin_bit_cast(bf16x2_t, b.y), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.z), __builtin_bit_cast(bf16x2_t, b.z), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a.w), __builtin_bit_cast(bf16x2_t, b.w), acc, false);
    return acc;
  }
};

// acc[0 .. VN) += ca * (chunk a) + cb * (chunk b): two rows of an accumulation at a time.  bfloat16: the two coefficients are
// rounded to one bfloat16 pair and v_perm_b32 pairs up the rows' elements, so that v_dot2c_f32_bf16 does both products with
// no conversion (4 instructions per 4 products; converting and multiplying singly costs 6 to 8)
template <typename T>
struct Axpy2;
template <>
struct Axpy2<float> {
  struct Coef {
    float a, b;
  };
  static __device__ __forceinline__ Coef coef(float a, float b) { return Coef{a, b}; }
  static __device__ __forceinline__ void run(float* acc, Coef c, const float4& ra, const float4& rb) {
    acc[0] += c.a * ra.x + c.b * rb.x;
    acc[1] += c.a * ra.y + c.b * rb.y;
    acc[2] += c.a * ra.z + c.b * rb.z;
    acc[3] += c.a * ra.w + c.b * rb.w;
  }
};
template <>
struct Axpy2<bf16_t> {
  typedef unsigned Coef;
  static __device__ __forceinline__ Coef coef(float a, float b) { return pack_bf16x2(a, b); }
  static __device__ __forceinline__ void pair(float* acc, unsigned c, unsigned a, unsigned b) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const unsigned lo = __builtin_amdgcn_perm(b, a, 0x05040100u);    // (a.even, b.even)
    const unsigned hi = __builtin_amdgcn_perm(b, a, 0x07060302u);    // (a.odd, b.odd)
    const bf16x2_t cc = __builtin_bit_cast(bf16x2_t, c);
    acc[0] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, lo), cc, acc[0], false);
    acc[1] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, hi), cc, acc[1], false);
  }
  static __device__ __forceinline__ void run(float* acc, Coef c, const uint4& ra, const uint4& rb) {
    pair(acc + 0, c, ra.x, rb.x);
    pair(acc + 2, c, ra.y, rb.y);
    pair(acc + 4, c, ra.z, rb.z);
    pair(acc + 6, c, ra.w, rb.w);
  }
};

}  // namespace htrvt
