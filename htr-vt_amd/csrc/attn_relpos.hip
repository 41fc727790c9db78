// attn_relpos.hip -- fused bfloat16 self-attention with the learned relative-position bias TABLE of the window-attention
// fork (model_window/model/HTR_VT.py:11-62 Attention, :113-154 Block._attend), forward and both backward launches.
//
// Same tiling, LDS images and MFMA orientation as attention.hip (see there); what differs is where the score bias comes
// from and where its gradient goes:
//   * the table [2P-1][heads] float32 (the reference parameter as stored, P = num_patches) is not expanded to a dense
//     [heads][N][N] bias: each workgroup stages its head's column in LDS (pre-multiplied by log2(e)) together with one
//     int "code" per token, and the bias of a (query, key) pair is formed in registers:
//       full attention (window 0):  code(t) = t,                                 R = P
//       windowed (window ws):       pos = (t - shift) mod Np, Np = ceil(N / ws) ws,
//                                   code(t) = (pos / ws) * 2^16 + pos % ws,       R = ws
//       diff = code(key) - code(query); the pair attends iff |diff| < R, then it uses table entry diff + P - 1
//     (two tokens of different windows are >= 2^16 - ws apart); padding keys / queries of a ragged last tile carry codes
//     +-2^29: never inside a window.  Masked pairs score -1e30 (finite: an all-masked key tile for one query cannot
//     produce inf - inf in the online softmax; every query sees at least itself, which wipes what such a tile added).
//   * windowed attention: a staged tile that no query (forward, dQ) / key (dK dV) of the workgroup can see is skipped.
//   * d(table) without atomics and in a fixed order: the dQ launch sees every key of its query rows.  Its d(score) values
//     (in the pair layout of the accumulators: lane (r, half) = query q0 + r, register i = key 32 c + (i & 3) + 8 (i >> 2)
//     + 4 half) are summed per token DIAGONAL d = key - query -- each 32 x 32 block goes through a per-wave LDS scratch,
//     lane L sums diagonal L - 31 over the 32 queries in order and adds it to a per-wave diagonal array in tile order.  After the key loop the
//     workgroup maps diagonals to table entries (full: e = d + P - 1; windowed: d in {delta, delta +- Np} for delta =
//     e - P + 1, |delta| < ws: pairs across the cyclic wrap of the shifted windows) and writes one partial row of 2P-1
//     floats; a second small launch sums the rows of a head over (batch, query block) in a fixed order and ADDS the result
//     to dtable (the accumulate rule of parameter gradients).  Bitwise reproducible run to run.
#include <stdlib.h>

#include "attention_common.h"

using namespace htrvt;

namespace {

constexpr float MASKED2 = -1.0e30f;          // score (base-2 domain) of a pair outside the window / a padding key
constexpr int PAD_KEY = 1 << 29, PAD_QUERY = -(1 << 29);

struct RelParams {
  const bf16_t* qkv;
  bf16_t* out;         // forward output [B*N][h*hd]
  float* lse2;         // [B*h][N]
  const bf16_t* dout;  // backward: gradient of out
  const bf16_t* o;     // backward: forward output
  bf16_t* dqkv;        // backward: gradient of qkv
  const float* table;  // [2P-1][h] float32
  float* ws_rows;      // backward: [h][B][nqb][2P-1] partial d(table) rows, or NULL (no table gradient)
  int B, N, h;
  float sl2;           // scale * log2(e)
  float scale;
  int P, win, shift, Np, R;
  int ncode;           // tokens with a code in LDS: N rounded up to 128
};

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// code of token t (see the top of the file); t > N - 1: `pad`
__device__ __forceinline__ int token_code(const RelParams& p, int t, int pad) {
  if (t >= p.N) return pad;
  if (p.win <= 0) return t;
  int pos = t - p.shift;
  pos += pos < 0 ? p.Np : 0;
  const int w = pos / p.win;
  return (w << 16) + (pos - w * p.win);
}

// windows of the rolled sequence met by the tokens a .. b (a <= b < N): [lo, hi] and, for tokens before the shift, the last
// window (their rolled positions wrap to the end)
struct WinSet {
  int lo, hi;
  bool last;
};

__device__ __forceinline__ WinSet win_set(const RelParams& p, int a, int b) {
  WinSet s{0, -1, a < p.shift};
  if (b >= p.shift) {
    s.lo = (max(a, p.shift) - p.shift) / p.win;
    s.hi = (b - p.shift) / p.win;
  }
  return s;
}

__device__ __forceinline__ bool win_has(const WinSet& s, int w, int nw) {
  return (s.lo <= w && w <= s.hi) || (s.last && w == nw - 1);
}

// can some token of [a0, a1] attend to some token of [b0, b1]?  (workgroup-uniform; full attention: always)
__device__ __forceinline__ bool tiles_meet(const RelParams& p, int a0, int a1, int b0, int b1) {
  if (p.win <= 0) return true;
  const int nw = p.Np / p.win;
  const WinSet A = win_set(p, a0, a1), Bs = win_set(p, b0, b1);
  return max(A.lo, Bs.lo) <= min(A.hi, Bs.hi) || (A.last && win_has(Bs, nw - 1, nw)) || (Bs.last && win_has(A, nw - 1, nw));
}

// first staged tile >= t (of `nt`, `len` tokens each) that meets the tokens [a0, a1]; nt if none
__device__ __forceinline__ int next_live(const RelParams& p, int t, int nt, int len, int a0, int a1) {
  while (t < nt && !tiles_meet(p, a0, a1, t * len, min(t * len + len - 1, p.N - 1))) ++t;
  return t;
}

// token codes + the head's table column (times log2 e) into LDS; every thread of the workgroup takes part
__device__ __forceinline__ void stage_codes_table(const RelParams& p, int hh, int* codes, float* tabl) {
  for (int t = threadIdx.x; t < p.ncode; t += blockDim.x) codes[t] = token_code(p, t, PAD_KEY);
  for (int e = threadIdx.x; e < 2 * p.P - 1; e += blockDim.x) tabl[e] = p.table[(long long)e * p.h + hh] * LOG2E;
}

// base-2 score bias of the pair (query code cq, key code ck): table entry inside the window, MASKED2 outside
__device__ __forceinline__ float pair_bias(const RelParams& p, const float* tabl, int cq, int ck) {
  const int diff = ck - cq;
  const bool in = (unsigned)(diff + p.R - 1) < (unsigned)(2 * p.R - 1);
  const float b = tabl[in ? diff + p.P - 1 : 0];
  return in ? b : MASKED2;
}

template <int HD>
constexpr int kv_bytes() { return 2 * 2 * KT * HD * 2; }       // [2][K tile | V tile]

__host__ __device__ inline int tab_floats(int P) { return (2 * P - 1 + 3) / 4 * 4; }

// -------------------------------------------------------------------------------------------------------------------
// forward: attention.hip attn_fwd_kernel with the bias from the table
// -------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, 2) void relpos_fwd_kernel(const RelParams p) {
  constexpr int NTH = 256, QB = 128;
  constexpr int TILE_B = KT * HD * 2;
  constexpr int NS = HD / 16;
  constexpr int ND = HD / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][K tile | V tile] | codes[ncode] | table column
  int* codes = reinterpret_cast<int*>(smem + kv_bytes<HD>());
  float* tabl = reinterpret_cast<float*>(codes + p.ncode);

  const int nqb = (p.N + QB - 1) / QB;
  const int last = p.N - 1;
  const int total = gridDim.x;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  const int bh = id / nqb, qb = id - bh * nqb;
  const int b = bh / p.h, hh = bh - b * p.h;
  const long long ld = 3ll * p.h * HD;
  const bf16_t* qbase = p.qkv + (long long)b * p.N * ld + hh * HD;
  const bf16_t* kbase = qbase + p.h * HD;
  const bf16_t* vbase = kbase + p.h * HD;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const LaneAddr<HD> la = lane_addr<HD>(lane);
  const int q0 = qb * QB + wave * 32;
  const int qrow = min(q0 + r, last);
  const int qa = qb * QB, qz = min(qa + QB - 1, last);      // the workgroup's real queries

  bf16x8_t qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    qf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(qbase + (long long)qrow * ld + 16 * s + 8 * hf));

  const int nt = (p.N + KT - 1) / KT;
  int t = next_live(p, 0, nt, KT, qa, qz);
  TileStage<HD, NTH> sk, sv;
  sk.issue(kbase, ld, t * KT, last);
  sv.issue(vbase, ld, t * KT, last);
  stage_codes_table(p, hh, codes, tabl);
  sk.commit(smem);
  sv.commit(smem + TILE_B);
  __syncthreads();
  const int cq = q0 + r <= last ? codes[q0 + r] : PAD_QUERY;

  f32x16_t o[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int it = 0; t < nt; ++it) {
    const char* kt = smem + (it & 1) * 2 * TILE_B;
    const char* vt = kt + TILE_B;
    char* nxt = smem + ((it + 1) & 1) * 2 * TILE_B;
    const int tl = next_live(p, t + 1, nt, KT, qa, qz);
    const int tn = tl < nt ? tl : t;       // the last iteration re-stages its own tile into the idle buffer
    sk.issue(kbase, ld, tn * KT, last);
    sv.issue(vbase, ld, tn * KT, last);
    f32x16_t st[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int i = 0; i < 16; ++i) st[c][i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s)
        st[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<HD>(kt, la, 32 * c, s), qf[s], st[c], 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int4 ck = *reinterpret_cast<const int4*>(codes + t * KT + 32 * c + 8 * g + 4 * hf);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float bv = pair_bias(p, tabl, cq, (&ck.x)[j]);
          const float sb = bv == MASKED2 ? MASKED2 : fmaf(st[c][4 * g + j], p.sl2, bv);
          st[c][4 * g + j] = sb;
          mx = fmaxf(mx, sb);
        }
      }
    mx = fmaxf(mx, xhalf(mx));
    const float mn = fmaxf(m, mx);
    float rs = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        st[c][i] = fast_exp2(st[c][i] - mn);
        rs += st[c][i];
      }
    if (__any(mn > m)) {
      const float alpha = fast_exp2(m - mn);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] *= alpha;
    }
    l += rs;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8_t pb = acc_frag(st[c], s);
#pragma unroll
        for (int d = 0; d < ND; ++d)
          o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<HD>(vt, la, 32 * c, s, d), pb, o[d], 0, 0, 0);
      }
    sk.commit(nxt);
    sv.commit(nxt + TILE_B);
    __syncthreads();
    t = tl;
  }

  l += xhalf(l);
  const float inv = 1.0f / l;
  if (q0 + r <= last) {
    store_lane_rows<ND>(o, p.out + ((long long)b * p.N + q0 + r) * ((long long)p.h * HD) + hh * HD, hf, inv);
    if (hf == 0 && p.lse2 != nullptr) p.lse2[(long long)bh * p.N + q0 + r] = m + log2f(l);
  }
}

// -------------------------------------------------------------------------------------------------------------------
// backward, first launch: dQ, delta = rowsum(dO * O), and the workgroup's partial row of d(table)
// -------------------------------------------------------------------------------------------------------------------
// hd 128: one workgroup per CU (the diagonal sums need more than the 256 VGPRs of two workgroups per CU: 5 spilled there)
template <int HD>
__global__ __launch_bounds__(256, HD >= 128 ? 1 : 2) void relpos_bwd_dq_kernel(const RelParams p, float* __restrict__ delta) {
  constexpr int NTH = 256, QB = 128;
  constexpr int TILE_B = KT * HD * 2;
  constexpr int NS = HD / 16, ND = HD / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // K/V tiles | codes | table column | 4 diagonal arrays
  int* codes = reinterpret_cast<int*>(smem + kv_bytes<HD>());
  float* tabl = reinterpret_cast<float*>(codes + p.ncode);
  const int nt = (p.N + KT - 1) / KT;
  const int ndiag = nt * KT + 32;                  // per wave: u = key - query + (wave's first query) + 31
  float* diag_all = tabl + tab_floats(p.P);

  const int nqb = (p.N + QB - 1) / QB;
  const int last = p.N - 1;
  const int total = gridDim.x;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  const int bh = id / nqb, qb = id - bh * nqb;
  const int b = bh / p.h, hh = bh - b * p.h;
  const long long ld = 3ll * p.h * HD, ldo = (long long)p.h * HD;
  const bf16_t* qbase = p.qkv + (long long)b * p.N * ld + hh * HD;
  const bf16_t* kbase = qbase + p.h * HD;
  const bf16_t* vbase = kbase + p.h * HD;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const LaneAddr<HD> la = lane_addr<HD>(lane);
  const int q0 = qb * QB + wave * 32;
  const int qa = qb * QB, qz = min(qa + QB - 1, last);
  const bool want_table = p.ws_rows != nullptr;
  float* diag = diag_all + wave * ndiag;
  float* blk = diag_all + 4 * ndiag + wave * (32 * 33);     // per-wave [32][33] d(score) block

  bf16x8_t qf[NS], dof[NS];
  float dl = 0.f;
  const int qrow = min(q0 + r, last);
  {
    const bf16_t* dorow = p.dout + ((long long)b * p.N + qrow) * ldo + hh * HD;
    const bf16_t* orow = p.o + ((long long)b * p.N + qrow) * ldo + hh * HD;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      qf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(qbase + (long long)qrow * ld + 16 * s + 8 * hf));
      Vec16<bf16_t> vd, vo;
      vd.raw = *reinterpret_cast<const uint4*>(dorow + 16 * s + 8 * hf);
      vo.raw = *reinterpret_cast<const uint4*>(orow + 16 * s + 8 * hf);
      dof[s] = __builtin_bit_cast(bf16x8_t, vd.raw);
#pragma unroll
      for (int j = 0; j < 8; ++j) dl = fmaf(vd.get(j), vo.get(j), dl);
    }
  }
  dl += xhalf(dl);
  const float lse = p.lse2[(long long)bh * p.N + qrow];
  if (hf == 0 && q0 + r <= last) delta[(long long)bh * p.N + q0 + r] = dl;

  int t = next_live(p, 0, nt, KT, qa, qz);
  TileStage<HD, NTH> sk, sv;
  sk.issue(kbase, ld, t * KT, last);
  sv.issue(vbase, ld, t * KT, last);
  stage_codes_table(p, hh, codes, tabl);
  if (want_table)
    for (int u = threadIdx.x; u < 4 * ndiag; u += NTH) diag_all[u] = 0.f;
  sk.commit(smem);
  sv.commit(smem + TILE_B);
  __syncthreads();
  // padding queries (q > last) get the query sentinel: every pair of theirs is masked, P = 0, d(score) = 0
  const int cq = q0 + r <= last ? codes[q0 + r] : PAD_QUERY;

  f32x16_t dq[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;

  for (int it = 0; t < nt; ++it) {
    const char* kt = smem + (it & 1) * 2 * TILE_B;
    const char* vt = kt + TILE_B;
    char* nxt = smem + ((it + 1) & 1) * 2 * TILE_B;
    const int tl = next_live(p, t + 1, nt, KT, qa, qz);
    const int tn = tl < nt ? tl : t;
    sk.issue(kbase, ld, tn * KT, last);
    sv.issue(vbase, ld, tn * KT, last);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      f32x16_t st, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = dp[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<HD>(kt, la, 32 * c, s), qf[s], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<HD>(vt, la, 32 * c, s), dof[s], dp, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int4 ck = *reinterpret_cast<const int4*>(codes + t * KT + 32 * c + 8 * g + 4 * hf);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float bv = pair_bias(p, tabl, cq, (&ck.x)[j]);
          const float pr = bv == MASKED2 ? 0.f : fast_exp2(fmaf(st[4 * g + j], p.sl2, bv - lse));
          st[4 * g + j] = pr * (dp[4 * g + j] - dl);          // d(score) = d(bias entry) of this pair
          dp[4 * g + j] = st[4 * g + j] * p.scale;             // dS
        }
      }
      if (want_table) {
        // d(score) of this 32 x 32 block -> the wave's scratch [query r][key kk] (kk = (i & 3) + 8 (i >> 2) + 4 half), then
        // lane L sums diagonal j = kk - r = L - 31 over r = 0 .. 31 in that order (lane 63: none)
#pragma unroll
        for (int i = 0; i < 16; ++i) blk[r * 33 + (i & 3) + 8 * (i >> 2) + 4 * hf] = st[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float acc = 0.f;
#pragma unroll 8
        for (int rr = 0; rr < 32; ++rr) {
          const int kk = rr + lane - 31;
          const float v = blk[rr * 33 + min(max(kk, 0), 31)];
          acc += (unsigned)kk < 32u ? v : 0.f;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();        // every lane has read the block before the next one is written
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // lane L of this step and lane L - 32 of the next one share a diagonal: volatile keeps the compiler from moving the
        // next step's read (a different address for THIS lane) above this write; the LDS serves one wave in order
        typedef __attribute__((address_space(3))) float lds_float;
        volatile lds_float* du = (volatile lds_float*)(diag + t * KT + 32 * c + lane);
        *du = *du + acc;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8_t dsb = acc_frag(dp, s);
#pragma unroll
        for (int d = 0; d < ND; ++d)
          dq[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<HD>(kt, la, 32 * c, s, d), dsb, dq[d], 0, 0, 0);
      }
    }
    sk.commit(nxt);
    sv.commit(nxt + TILE_B);
    __syncthreads();
    t = tl;
  }
  if (q0 + r <= last) store_lane_rows<ND>(dq, p.dqkv + ((long long)b * p.N + q0 + r) * ld + hh * HD, hf, 1.0f);

  if (want_table) {      // diagonals -> table entries, waves in order; one partial row of 2P-1 floats per workgroup
    const int ne = 2 * p.P - 1;
    float* row = p.ws_rows + ((long long)(hh * p.B + b) * nqb + qb) * ne;
    for (int e = threadIdx.x; e < ne; e += NTH) {
      const int dl0 = e - (p.P - 1);
      // diagonals of entry e: d0 (windowed: only inside the window), and across the cyclic wrap d0 +- Np (shifted windows)
      const bool in0 = p.win <= 0 || (dl0 > -p.win && dl0 < p.win);
      const bool wrap = in0 && p.win > 0 && p.shift > 0;
      float s = 0.f;
      for (int w = 0; w < 4; ++w) {
        const int u = dl0 + qa + 32 * w + 31;
        if (in0 && u >= 0 && u < ndiag) s += diag_all[w * ndiag + u];
        if (wrap && u + p.Np >= 0 && u + p.Np < ndiag) s += diag_all[w * ndiag + u + p.Np];
        if (wrap && u - p.Np >= 0 && u - p.Np < ndiag) s += diag_all[w * ndiag + u - p.Np];
      }
      row[e] = s;
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------
// backward, second launch: dK and dV (attention.hip attn_bwd_dkv_kernel with the bias from the table)
// -------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, 1) void relpos_bwd_dkv_kernel(const RelParams p, const float* __restrict__ delta) {
  constexpr int NTH = 256, KB = 128, QT = HD >= 128 ? 64 : 128;
  constexpr int TILE_B = QT * HD * 2;
  constexpr int STAGE_B = 2 * TILE_B + 2 * QT * 4 + 16;
  constexpr int NS = HD / 16, ND = HD / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][Q | dO | lse2 | delta | dump] | codes | table column
  int* codes = reinterpret_cast<int*>(smem + 2 * STAGE_B);
  float* tabl = reinterpret_cast<float*>(codes + p.ncode);

  const int nkb = (p.N + KB - 1) / KB;
  const int last = p.N - 1;
  const int total = gridDim.x;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  const int bh = id / nkb, kb = id - bh * nkb;
  const int b = bh / p.h, hh = bh - b * p.h;
  const long long ld = 3ll * p.h * HD, ldo = (long long)p.h * HD;
  const bf16_t* qbase = p.qkv + (long long)b * p.N * ld + hh * HD;
  const bf16_t* kbase = qbase + p.h * HD;
  const bf16_t* vbase = kbase + p.h * HD;
  const bf16_t* dobase = p.dout + (long long)b * p.N * ldo + hh * HD;
  const float* lsebase = p.lse2 + (long long)bh * p.N;
  const float* delbase = delta + (long long)bh * p.N;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const LaneAddr<HD> la = lane_addr<HD>(lane);
  const int k0 = kb * KB + wave * 32;
  const int ka = kb * KB, kz = min(ka + KB - 1, last);

  bf16x8_t kf[NS], vf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    kf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(kbase + (long long)min(k0 + r, last) * ld + 16 * s + 8 * hf));
    vf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(vbase + (long long)min(k0 + r, last) * ld + 16 * s + 8 * hf));
  }

  const int nt = (p.N + QT - 1) / QT;
  int t = next_live(p, 0, nt, QT, ka, kz);
  TileStage<HD, NTH, QT> sq, sd;
  const float* cbase = threadIdx.x < QT ? lsebase + threadIdx.x : (threadIdx.x < 2 * QT ? delbase + (threadIdx.x - QT) : lsebase);
  const int cslot = threadIdx.x < 2 * QT ? threadIdx.x : 2 * QT;
  const int cidx = threadIdx.x < QT ? (int)threadIdx.x : (threadIdx.x < 2 * QT ? (int)threadIdx.x - QT : 0);
  const bool is_lse = threadIdx.x < QT;
  sq.issue(qbase, ld, t * QT, last);
  sd.issue(dobase, ldo, t * QT, last);
  float sc = cbase[min(t * QT + cidx, last) - cidx];
  if (is_lse && t * QT + cidx > last) sc = INFINITY;
  stage_codes_table(p, hh, codes, tabl);
  sq.commit(smem);
  sd.commit(smem + TILE_B);
  reinterpret_cast<float*>(smem + 2 * TILE_B)[cslot] = sc;
  __syncthreads();
  const int ckey = codes[k0 + r];          // a padding key's pairs are masked; its row is not stored

  f32x16_t dk[ND], dv[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dk[d][i] = dv[d][i] = 0.f;

  for (int it = 0; t < nt; ++it) {
    const char* qt = smem + (it & 1) * STAGE_B;
    const char* dot = qt + TILE_B;
    const float* cst = reinterpret_cast<const float*>(qt + 2 * TILE_B);
    char* nxt = smem + ((it + 1) & 1) * STAGE_B;
    const int tl = next_live(p, t + 1, nt, QT, ka, kz);
    const int tn = tl < nt ? tl : t;
    sq.issue(qbase, ld, tn * QT, last);
    sd.issue(dobase, ldo, tn * QT, last);
    sc = cbase[min(tn * QT + cidx, last) - cidx];
    if (is_lse && tn * QT + cidx > last) sc = INFINITY;
#pragma unroll
    for (int c = 0; c < QT / 32; ++c) {
      f32x16_t st, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = dp[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<HD>(qt, la, 32 * c, s), kf[s], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<HD>(dot, la, 32 * c, s), vf[s], dp, 0, 0, 0);
      }
      // accumulator register i is query t QT + 32 c + (i & 3) + 8 (i >> 2) + 4 hf
      static_for<0, 4>([&](auto G) {
        constexpr int g = decltype(G)::value;
        const float4 ls = *reinterpret_cast<const float4*>(cst + 32 * c + 8 * g + 4 * hf);
        const float4 de = *reinterpret_cast<const float4*>(cst + QT + 32 * c + 8 * g + 4 * hf);
        const int4 cqv = *reinterpret_cast<const int4*>(codes + t * QT + 32 * c + 8 * g + 4 * hf);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dev[4] = {de.x, de.y, de.z, de.w};
        const int cqa[4] = {cqv.x, cqv.y, cqv.z, cqv.w};
        static_for<0, 4>([&](auto J) {
          constexpr int j = decltype(J)::value, i = 4 * g + j;
          const float bv = pair_bias(p, tabl, cqa[j], ckey);
          // (a padding query carries lse2 = +inf: pr = 0)
          const float pr = bv == MASKED2 ? 0.f : fast_exp2(fmaf(st[i], p.sl2, bv - lsv[j]));
          const float dsu = pr * (dp[i] - dev[j]);
          st[i] = pr;
          dp[i] = dsu * p.scale;
        });
      });
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8_t pb = acc_frag(st, s), dsb = acc_frag(dp, s);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          dv[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<HD>(dot, la, 32 * c, s, d), pb, dv[d], 0, 0, 0);
          dk[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<HD>(qt, la, 32 * c, s, d), dsb, dk[d], 0, 0, 0);
        }
      }
    }
    sq.commit(nxt);
    sd.commit(nxt + TILE_B);
    reinterpret_cast<float*>(nxt + 2 * TILE_B)[cslot] = sc;
    __syncthreads();
    t = tl;
  }
  if (k0 + r <= last) {
    bf16_t* grow = p.dqkv + ((long long)b * p.N + k0 + r) * ld + hh * HD;
    store_lane_rows<ND>(dk, grow + p.h * HD, hf, 1.0f);
    store_lane_rows<ND>(dv, grow + 2 * p.h * HD, hf, 1.0f);
  }
}

// dtable[e][hh] += sum over the rows of head hh (batch-major, then query block), in that order: 4 groups of 64 threads take
// every 4th row, then the four partial sums are added in group order
__global__ __launch_bounds__(256) void relpos_dtable_kernel(const float* __restrict__ rows, float* __restrict__ dtable,
                                                            int nrows, int ne, int h) {
  __shared__ float part[4][64];
  const int hh = blockIdx.y;
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
  float s = 0.f;
  if (e < ne) {
    const float* base = rows + (long long)hh * nrows * ne + e;
    for (int rw = grp; rw < nrows; rw += 4) s += base[(long long)rw * ne];
  }
  part[grp][threadIdx.x & 63] = s;
  __syncthreads();
  if (grp == 0 && e < ne) {
    const int x = threadIdx.x;
    dtable[(long long)e * h + hh] += ((part[0][x] + part[1][x]) + part[2][x]) + part[3][x];
  }
}

constexpr int MAX_P = 2048;
constexpr int LDS_MAX = 160 * 1024;

// geometry / shape check shared by every entry point; 0 = fine, else the error is set
int check_geometry(int N, int hd, int dtype, int P, int win, int shift, const char* what) {
  if (dtype != HTRVT_BF16) { set_error("%s: bfloat16 only (float32: htrvt_relpos_bias_fwd + GEMMs)", what); return -1; }
  if (hd != 64 && hd != 128) { set_error("%s: head dim %d not in {64, 128}", what, hd); return -1; }
  if (N < 32) { set_error("%s: N=%d < 32", what, N); return -1; }
  if (P > MAX_P) { set_error("%s: num_patches=%d > %d (the table column and token codes live in LDS)", what, P, MAX_P); return -1; }
  if (N > P) { set_error("%s: N=%d exceeds num_patches=%d (the table has 2P-1 entries)", what, N, P); return -1; }
  if (win < 0) { set_error("%s: window=%d < 0", what, win); return -1; }
  if (win == 0 && shift != 0) { set_error("%s: shift=%d without a window", what, shift); return -1; }
  if (win > 0) {
    if (shift < 0 || shift >= win) { set_error("%s: shift=%d outside [0, window=%d)", what, shift, win); return -1; }
    const int Np = ceil_div(N, win) * win;
    if (shift > 0 && Np < 2 * win) {
      set_error("%s: a shifted window needs at least two windows (N=%d, window=%d)", what, N, win);
      return -1;
    }
  }
  return 0;
}

RelParams make_params(const void* qkv, const float* table, int B, int N, int heads, float scale, int P, int win, int shift) {
  RelParams p{};
  p.qkv = (const bf16_t*)qkv;
  p.table = table;
  p.B = B; p.N = N; p.h = heads;
  p.scale = scale;
  p.sl2 = scale * LOG2E;
  p.P = P; p.win = win; p.shift = win > 0 ? shift : 0;
  p.Np = win > 0 ? ceil_div(N, win) * win : N;
  p.R = win > 0 ? win : P;
  p.ncode = ceil_div(N, 128) * 128;
  return p;
}

int fwd_lds(int hd, const RelParams& p) { return (hd == 128 ? kv_bytes<128>() : kv_bytes<64>()) + 4 * p.ncode + 4 * tab_floats(p.P); }
int dq_lds(int hd, const RelParams& p) { return fwd_lds(hd, p) + 4 * 4 * (ceil_div(p.N, KT) * KT + 32) + 4 * 4 * 32 * 33; }
int dkv_lds(int hd, const RelParams& p) {
  const int QT = hd >= 128 ? 64 : 128;
  return 2 * (2 * QT * hd * 2 + 2 * QT * 4 + 16) + 4 * p.ncode + 4 * tab_floats(p.P);
}

template <int HD>
int launch_fwd(const RelParams& p, hipStream_t st) {
  static bool attr_done[64] = {};       // per device: the LDS attribute is set on the device that launches
  auto kern = relpos_fwd_kernel<HD>;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!attr_done[dev]) {
    if (int rc = set_lds(kern, LDS_MAX, "attn_relpos_fwd")) return rc;
    attr_done[dev] = true;
  }
  hipLaunchKernelGGL(kern, dim3(p.B * p.h * ceil_div(p.N, 128)), dim3(256), fwd_lds(HD, p), st, p);
  return check_launch("attn_relpos_fwd");
}

template <int HD>
int launch_bwd(const RelParams& p, float* delta, float* dtable, hipStream_t st) {
  static bool attr_done[64] = {};       // per device, as in launch_fwd
  auto kq = relpos_bwd_dq_kernel<HD>;
  auto kkv = relpos_bwd_dkv_kernel<HD>;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!attr_done[dev]) {
    if (int rc = set_lds(kq, LDS_MAX, "attn_relpos_bwd_dq")) return rc;
    if (int rc = set_lds(kkv, LDS_MAX, "attn_relpos_bwd_dkv")) return rc;
    attr_done[dev] = true;
  }
  const int nqb = ceil_div(p.N, 128);
  const dim3 grid(p.B * p.h * nqb);
  hipLaunchKernelGGL(kq, grid, dim3(256), dq_lds(HD, p), st, p, delta);
  hipLaunchKernelGGL(kkv, grid, dim3(256), dkv_lds(HD, p), st, p, (const float*)delta);
  if (dtable != nullptr) {
    const int ne = 2 * p.P - 1;
    hipLaunchKernelGGL(relpos_dtable_kernel, dim3(ceil_div(ne, 64), p.h), dim3(256), 0, st, (const float*)p.ws_rows, dtable,
                       p.B * nqb, ne, p.h);
  }
  return check_launch("attn_relpos_bwd");
}

}  // namespace

extern "C" int htrvt_attn_relpos_supported(int N, int hd, int dtype, int num_patches, int window, int shift) {
  return check_geometry(N, hd, dtype, num_patches, window, shift, "htrvt_attn_relpos") == 0 ? 1 : 0;
}

extern "C" int64_t htrvt_attn_relpos_bwd_workspace_floats(int B, int N, int heads, int num_patches, int window, int shift) {
  if (check_geometry(N, 128, HTRVT_BF16, num_patches, window, shift, "htrvt_attn_relpos_bwd_workspace_floats")) return -1;
  if (B <= 0 || heads <= 0) { set_error("htrvt_attn_relpos_bwd_workspace_floats: B=%d heads=%d", B, heads); return -1; }
  return (int64_t)heads * B * ceil_div(N, 128) * (2 * num_patches - 1);
}

extern "C" int htrvt_attn_relpos_fwd(const void* qkv, const float* table, void* out, float* lse2, int B, int N, int heads,
                                     int hd, float scale, int num_patches, int window, int shift, int dtype, void* stream) {
  HTRVT_REQUIRE(qkv && table && out, "htrvt_attn_relpos_fwd: null operand");
  if (int rc = check_geometry(N, hd, dtype, num_patches, window, shift, "htrvt_attn_relpos_fwd")) return rc;
  HTRVT_REQUIRE(B > 0 && heads > 0, "htrvt_attn_relpos_fwd: B=%d heads=%d", B, heads);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_relpos_fwd: qkv too large");
  RelParams p = make_params(qkv, table, B, N, heads, scale, num_patches, window, shift);
  p.out = (bf16_t*)out;
  p.lse2 = lse2;
  HTRVT_REQUIRE(fwd_lds(hd, p) <= LDS_MAX, "htrvt_attn_relpos_fwd: %d B of LDS", fwd_lds(hd, p));
  hipStream_t st = (hipStream_t)stream;
  return hd == 128 ? launch_fwd<128>(p, st) : launch_fwd<64>(p, st);
}

extern "C" int htrvt_attn_relpos_bwd(const void* qkv, const float* table, const void* out, const void* dout, const float* lse2,
                                     float* delta, void* dqkv, float* dtable, float* workspace, int B, int N, int heads, int hd,
                                     float scale, int num_patches, int window, int shift, int dtype, void* stream) {
  HTRVT_REQUIRE(qkv && table && out && dout && lse2 && delta && dqkv, "htrvt_attn_relpos_bwd: null operand");
  HTRVT_REQUIRE(dtable == nullptr || workspace != nullptr, "htrvt_attn_relpos_bwd: dtable needs the workspace");
  if (int rc = check_geometry(N, hd, dtype, num_patches, window, shift, "htrvt_attn_relpos_bwd")) return rc;
  HTRVT_REQUIRE(B > 0 && heads > 0, "htrvt_attn_relpos_bwd: B=%d heads=%d", B, heads);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_relpos_bwd: qkv too large");
  RelParams p = make_params(qkv, table, B, N, heads, scale, num_patches, window, shift);
  p.o = (const bf16_t*)out;
  p.dout = (const bf16_t*)dout;
  p.lse2 = const_cast<float*>(lse2);
  p.dqkv = (bf16_t*)dqkv;
  p.ws_rows = dtable != nullptr ? workspace : nullptr;
  HTRVT_REQUIRE(dq_lds(hd, p) <= LDS_MAX && dkv_lds(hd, p) <= LDS_MAX, "htrvt_attn_relpos_bwd: %d / %d B of LDS",
                dq_lds(hd, p), dkv_lds(hd, p));
  hipStream_t st = (hipStream_t)stream;
  return hd == 128 ? launch_bwd<128>(p, delta, dtable, st) : launch_bwd<64>(p, delta, dtable, st);
}
