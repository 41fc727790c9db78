// attention_common.h -- tile staging, LDS fragment reads and small helpers of the fused attention kernels
// (attention_impl.h, which describes the CDNA4 mapping these serve).
#pragma once

#include <type_traits>

#include "gemm_common.h"

namespace {

using namespace htrvt;

constexpr int KT = 64;          // keys (forward, dQ role) or queries (dK/dV role) per staged tile
constexpr float LOG2E = 1.44269504088896340736f;

// byte offset of 16-byte chunk `ch` of row `row` in a [rows][HD] bfloat16 LDS tile
template <int HD>
__device__ __forceinline__ int lds_off(int row, int ch) {
  if constexpr (HD == 128) return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  else if constexpr (HD == 64) return 128 * row + 16 * (ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)));
  else return 64 * row + 16 * (ch ^ ((row >> 2) & 3));
}

typedef __attribute__((address_space(3))) s16x4_t* lds_tr_ptr;

// compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N-1.  Element indices of the accumulator vectors are
// constants from the start this way; with `#pragma unroll` loops whose body holds a store or an atomic the vectors were
// indexed dynamically for a while and ended up in scratch memory.
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// Per-lane address constants of the two fragment reads.  lds_off's XOR term depends only on the low four bits of the tile
// row, which are lane bits in both reads (row0 is a multiple of 32, 16 s a multiple of 16), and the chunk index is a
// compile-time part OR-ed with a lane part on disjoint bits -- so every fragment address is
//     (lane constant) XOR (compile-time constant) + (compile-time constant),
// one v_xor per distinct (s) / (dt) instead of the full shift / mask / xor chain per read (the kernels are VALU-bound
// beside their MFMAs).  tools/lds_bank_check.py checks these forms against lds_off for every lane.
template <int HD>
struct LaneAddr {
  int rowb;        // row read:  lds_off(row0 + r, 2 s + h)              = (rowb ^ 32 s) + ROWB row0
  int trb0, trb1;  // transposed: lds_off(row0 + 16 s + 4 h + q [+ 8], 4 dt + 2 g + (p >> 1)) + 8 (p & 1)
                   //                                                    = (trb ^ 64 dt) + ROWB (row0 + 16 s)
};

template <int HD>
__device__ __forceinline__ LaneAddr<HD> lane_addr(int lane) {
  const int h = lane >> 5, g = (lane >> 4) & 1, i = lane & 15, q = i >> 2, p = i & 3;
  LaneAddr<HD> la;
  la.rowb = lds_off<HD>(lane & 31, h);
  la.trb0 = lds_off<HD>(4 * h + q, 2 * g + (p >> 1)) + 8 * (p & 1);
  la.trb1 = lds_off<HD>(4 * h + q + 8, 2 * g + (p >> 1)) + 8 * (p & 1);
  return la;
}

// A operand (rows = 32 consecutive columns of the tile starting at 32*dt, k = 16 tile rows in accumulator-as-operand
// order: element j of lane half h is tile row row0 + 16 s + 8 (j >> 2) + 4 h + (j & 3)) by two transposed reads
template <int HD>
__device__ __forceinline__ bf16x8_t tr_frag(const char* tile, const LaneAddr<HD>& la, int row0, int s, int dt) {
  constexpr int ROWB = HD * 2;
  const int add = ROWB * (row0 + 16 * s);
  const s16x4_t r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(tile + ((la.trb0 ^ (64 * dt)) + add)));
  const s16x4_t r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(tile + ((la.trb1 ^ (64 * dt)) + add)));
  const s16x8_t r = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
  return __builtin_bit_cast(bf16x8_t, r);
}

// row operand: lane (r = lane & 31, h = lane >> 5) takes elements 16 s + 8 h .. + 7 of tile row row0 + r
template <int HD>
__device__ __forceinline__ bf16x8_t row_frag(const char* tile, const LaneAddr<HD>& la, int row0, int s) {
  constexpr int ROWB = HD * 2;
  const uint4 v = *reinterpret_cast<const uint4*>(tile + ((la.rowb ^ (32 * s)) + ROWB * row0));
  return __builtin_bit_cast(bf16x8_t, v);
}

// registers 8 s .. 8 s + 7 of a 32x32 accumulator tile, rounded to bfloat16: the operand of a following MFMA that
// contracts over the tile's ROW index
__device__ __forceinline__ bf16x8_t acc_frag(const f32x16_t& x, int s) {
  uint4 v;
  v.x = pack_bf16x2(x[8 * s + 0], x[8 * s + 1]);
  v.y = pack_bf16x2(x[8 * s + 2], x[8 * s + 3]);
  v.z = pack_bf16x2(x[8 * s + 4], x[8 * s + 5]);
  v.w = pack_bf16x2(x[8 * s + 6], x[8 * s + 7]);
  return __builtin_bit_cast(bf16x8_t, v);
}

// staging of one [KT][HD] tile: global -> registers (issue) ... registers -> LDS (commit), NTH threads
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));   // a first-class 16-byte vector: HIP's uint4 is a struct whose
                                                                    // copies are memcpys, which kept the staged tile in scratch
                                                                    // memory whenever a store or an atomic sat in between
template <int HD, int NTH, int ROWS = KT>
struct TileStage {
  static constexpr int CPR = HD / 8;                 // 16-byte chunks per row
  static constexpr int NL = ROWS * CPR / NTH;        // loads per thread
  static_assert(ROWS * CPR % NTH == 0 && NL >= 1 && NL <= 8, "tile must divide over the threads, at most 8 loads each");
  u32x4_t r0, r1, r2, r3, r4, r5, r6, r7;

  static __device__ __forceinline__ int row_of(int u) { return (threadIdx.x + NTH * u) / CPR; }
  static __device__ __forceinline__ int ch_of(int u) { return (threadIdx.x + NTH * u) % CPR; }
  static __device__ __forceinline__ u32x4_t ld16(const bf16_t* base, long long ld, int row, int ch) {
    return *reinterpret_cast<const u32x4_t*>(base + (long long)row * ld + ch * 8);
  }
  static __device__ __forceinline__ void st16(char* tile, int u, const u32x4_t& v) {
    *reinterpret_cast<u32x4_t*>(tile + lds_off<HD>(row_of(u), ch_of(u))) = v;
  }

  // rows past `last` (the sequence's last token: a partial final tile) re-read that row -- always valid memory; whatever
  // they contribute is masked by the caller (scores of padding keys -> -inf / probabilities of padding queries -> 0)
  __device__ __forceinline__ void issue(const bf16_t* base, long long ld, int row0, int last) {
    r0 = ld16(base, ld, min(row0 + row_of(0), last), ch_of(0));
    if constexpr (NL > 1) r1 = ld16(base, ld, min(row0 + row_of(1), last), ch_of(1));
    if constexpr (NL > 2) r2 = ld16(base, ld, min(row0 + row_of(2), last), ch_of(2));
    if constexpr (NL > 3) r3 = ld16(base, ld, min(row0 + row_of(3), last), ch_of(3));
    if constexpr (NL > 4) r4 = ld16(base, ld, min(row0 + row_of(4), last), ch_of(4));
    if constexpr (NL > 5) r5 = ld16(base, ld, min(row0 + row_of(5), last), ch_of(5));
    if constexpr (NL > 6) r6 = ld16(base, ld, min(row0 + row_of(6), last), ch_of(6));
    if constexpr (NL > 7) r7 = ld16(base, ld, min(row0 + row_of(7), last), ch_of(7));
  }
  __device__ __forceinline__ void commit(char* tile) const {
    st16(tile, 0, r0);
    if constexpr (NL > 1) st16(tile, 1, r1);
    if constexpr (NL > 2) st16(tile, 2, r2);
    if constexpr (NL > 3) st16(tile, 3, r3);
    if constexpr (NL > 4) st16(tile, 4, r4);
    if constexpr (NL > 5) st16(tile, 5, r5);
    if constexpr (NL > 6) st16(tile, 6, r6);
    if constexpr (NL > 7) st16(tile, 7, r7);
  }
};

// v_exp_f32 directly: every argument here is <= ~0 (a score minus its row maximum / log-sum-exp), results below 2^-126
// flush to zero, which is what a probability that small is worth; exp2f() would wrap the instruction in range scaling
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float xhalf(float v) { return __shfl_xor(v, 32, 64); }   // the other 32-lane half's value

// O[row][d] of a lane-per-row accumulator set: lane (r, hf) owns memory row `rowptr`, accumulator tile d register i is
// column 32 d + (i & 3) + 8 (i >> 2) + 4 hf: four consecutive columns per register quad -> 8-byte stores
template <int ND>
__device__ __forceinline__ void store_lane_rows(const f32x16_t (&acc)[ND], bf16_t* rowptr, int hf, float mul) {
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint2 v;
      v.x = pack_bf16x2(acc[d][4 * g + 0] * mul, acc[d][4 * g + 1] * mul);
      v.y = pack_bf16x2(acc[d][4 * g + 2] * mul, acc[d][4 * g + 3] * mul);
      *reinterpret_cast<uint2*>(rowptr + 32 * d + 8 * g + 4 * hf) = v;
    }
}

}  // namespace
