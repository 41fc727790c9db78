// window_attn_impl.h -- the one form of the window attention kernels that keep their scores on the VALU: lgp.hip's 1-D
// windows of at most 16 tokens (LPR = 4 lanes per row) and swin.hip's 2-D windows of at most 32 tokens (LPR = 2).
// One wave per (image, window, head).  Lane = (row = lane / LPR, part = lane % LPR): the lane owns the 16-byte chunks
// c = LPR i + part of its row's head slice (any partition of the head dimension serves a dot product; this one makes the
// lanes of a row read contiguous bytes).  k / v rows (and q / dO rows in the backward) are staged in LDS in their storage
// type, one 16-byte chunk of padding per row so that the rows of a store spread over all banks; reads of a row are
// broadcasts.  Scores are chunk dot products summed over the row's lanes by DPP, the softmax stays in registers, and every
// accumulation (P v, dS k, dS^T q, P^T dO) takes two rows at a time.  The backward leaves P and dS in LDS as
// [ROWS][ROWS + 1] floats and reads its coefficients back from there, so that its row loops need no full unrolling (fully
// unrolled they took every VGPR and ran slower).
// Here: the chunk arithmetic, the geometry, the lane sum, the row helpers, the one forward kernel and the host-side dispatch.
// A file supplies what differs: its "window source" (which token a window slot is, where rows that are no token come from,
// what is added to a score) and its backward kernel.  The backward kernels' phases (scores and dP, softmax to P and dS, dq,
// dk / dv, the stores) are written in each kernel, NOT as functions here: hipcc simplifies a __device__ function on its own
// before it inlines it, and with the phases here float32 gradients changed in the last bits (other products fused or packed)
// and two backward launches ran 0.9 % and 3.8 % slower.  In the kernels they compile to the streams they had.
#pragma once
#include <type_traits>

#include "common.h"

namespace htrvt {

// ------------------------------------------------------------------ arithmetic on 16-byte chunks as they are stored
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

// ------------------------------------------------------------------ geometry, lane sum, rows in and out
template <typename T, int HD, int LPR_>
struct WinAttnGeom {
  using V = Vec16<T>;
  using Raw = decltype(V().raw);
  static constexpr int LPR = LPR_;         // lanes per row: 4 or 2
  static constexpr int ROWS = 64 / LPR;    // rows of the largest window
  static constexpr int VN = V::N;          // elements per 16-byte chunk
  static constexpr int CPR = HD / VN;      // chunks per row
  static constexpr int CH = CPR / LPR;     // chunks per lane
  static constexpr int EPL = CH * VN;      // elements per lane
  static constexpr int RS = CPR + 1;       // LDS row stride in chunks
  static constexpr int MAT = ROWS * RS;    // chunks per staged matrix
};

// sum over the LPR lanes of a row, result in all of them
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  if constexpr (LPR == 4)
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true)); // quad_perm [2,3,0,1]
  return v;
}

// the lane's chunks of the row at `src`, into registers
template <class G>
__device__ __forceinline__ void load_row(typename G::Raw* regs, const typename G::Raw* src, int part) {
#pragma unroll
  for (int i = 0; i < G::CH; ++i) regs[i] = src[i * G::LPR + part];
}

// the lane's chunks of the row at `src`, into row `row` of the staged matrix `mat`
template <class G>
__device__ __forceinline__ void stage_row(typename G::Raw* mat, int row, int part, const typename G::Raw* src) {
#pragma unroll
  for (int i = 0; i < G::CH; ++i) mat[row * G::RS + i * G::LPR + part] = src[i * G::LPR + part];
}

// the lane's EPL floats, converted, into its chunks of the row at `dst`
template <class G>
__device__ __forceinline__ void store_chunks(typename G::Raw* dst, int part, const float* v) {
#pragma unroll
  for (int i = 0; i < G::CH; ++i) {
    typename G::V a;
#pragma unroll
    for (int e = 0; e < G::VN; ++e) a.set(e, v[i * G::VN + e]);
    dst[i * G::LPR + part] = a.raw;
  }
}

// the score of a window that adds nothing to scale q.k (a source with a bias or a mask passes a functor that adds them)
struct PlainScore {
  __device__ __forceinline__ float operator()(float qk, int) const { return qk; }
};

// ------------------------------------------------------------------ forward kernel
// One unit (image, window, head) per wave.  The window source `src` supplies
//   LPR, PADS               lanes per row; whether a window has rows that are no token
//   Lds                     what else its scores need in LDS, per wave (an empty struct: nothing is declared)
//   heads                   heads of the model: D = heads HD
//   unit(u, units, row)     what the wave's unit u and the lane's row are: .head, .tok (the token's row of qkv / out), .n (rows
//                           of the window), .rowact (the row is one of them), .real (it is a token)
//   stage_extras(ext, x, lane)            fills the wave's Lds, before the barrier
//   pad_row<G>(kl, vl, x, row, part)      stages the k / v row of a row that is no token (PADS only)
//   score(ext, x)           the functor (scale q.k, j) -> score of key row j
// All ROWS slots are unrolled under the `j < n` guard, so that s[] stays in registers.  The loops stand in the kernel itself:
// moved into a __device__ function, unchanged, they compile to a schedule with 10 to 22 more VGPRs in the float32 instances.
template <typename T, int HD, int WPB, class Src>
__global__ __launch_bounds__(64 * WPB) void window_attn_fwd_kernel(const Src src, const T* __restrict__ qkv,
                                                                   T* __restrict__ out, float scale, long long units) {
  using G = WinAttnGeom<T, HD, Src::LPR>;
  using Raw = typename G::Raw;
  __shared__ Raw lds[WPB][2][G::MAT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = lane / G::LPR, part = lane % G::LPR;
  typename Src::Lds* ext = nullptr;
  if constexpr (!std::is_empty_v<typename Src::Lds>) {
    __shared__ typename Src::Lds extras[WPB];
    ext = &extras[wv];
  }
  const auto x = src.unit((long long)blockIdx.x * WPB + wv, units, row);
  const int D = src.heads * HD;
  Raw* kl = lds[wv][0];
  Raw* vl = lds[wv][1];
  src.stage_extras(ext, x, lane);
  Raw q[G::CH];
#pragma unroll
  for (int i = 0; i < G::CH; ++i) q[i] = Raw{};
  if (x.real) {
    const Raw* row3 = reinterpret_cast<const Raw*>(qkv + x.tok * 3 * D + x.head * HD);
    load_row<G>(q, row3, part);
    stage_row<G>(kl, row, part, row3 + D / G::VN);
    stage_row<G>(vl, row, part, row3 + 2 * D / G::VN);
  } else if constexpr (Src::PADS) {
    if (x.rowact) src.template pad_row<G>(kl, vl, x, row, part);
  }
  __syncthreads();

  const auto score = src.score(ext, x);
  float s[G::ROWS];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < G::ROWS; ++j) {
    s[j] = -INFINITY;
    if (j < x.n) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < G::CH; ++i) acc = ChunkDot<T>::run(acc, q[i], kl[j * G::RS + i * G::LPR + part]);
      s[j] = score(row_sum<G::LPR>(acc) * scale, j);
      m = fmaxf(m, s[j]);
    }
  }
  float o[G::EPL];
#pragma unroll
  for (int e = 0; e < G::EPL; ++e) o[e] = 0.f;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < G::ROWS; j += 2) {
    if (j < x.n) {
      const bool two = j + 1 < x.n;        // an odd window's last row goes alone (its partner: the same row, weight 0)
      const float p0 = __expf(s[j] - m), p1 = two ? __expf(s[j + 1] - m) : 0.f;
      sum += p0 + p1;
      const auto c = Axpy2<T>::coef(p0, p1);
      const int j1 = two ? j + 1 : j;
#pragma unroll
      for (int i = 0; i < G::CH; ++i)
        Axpy2<T>::run(&o[i * G::VN], c, vl[j * G::RS + i * G::LPR + part], vl[j1 * G::RS + i * G::LPR + part]);
    }
  }
  if (x.real) {
    const float inv = 1.0f / sum;
#pragma unroll
    for (int e = 0; e < G::EPL; ++e) o[e] *= inv;
    store_chunks<G>(reinterpret_cast<Raw*>(out + x.tok * D + x.head * HD), part, o);
  }
}

}  // namespace htrvt

// ------------------------------------------------------------------ host side
// Each kernel has a table of the (dtype, hd) it serves and its waves per workgroup there: a macro TABLE(X) that lists
// X(T, HD, WPB) rows.  TABLE(WINDOW_ATTN_ROW) inside an entry point with `dtype` and `hd` in scope runs
// WINDOW_ATTN_LAUNCH(T, HD, WPB), which the entry point defines around the call, for the row that matches.
#define WINDOW_ATTN_ROW(T, HD, WPB) \
  if (dtype == (sizeof(T) == 2 ? HTRVT_BF16 : HTRVT_F32) && hd == HD) WINDOW_ATTN_LAUNCH(T, HD, WPB);
