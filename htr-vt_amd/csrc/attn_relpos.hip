// attn_relpos.hip -- fused bfloat16 self-attention with the learned relative-position bias TABLE of the window-attention
// fork (model_window/model/HTR_VT.py:11-62 Attention, :113-154 Block._attend), forward and both backward launches.
//
// The kernels are those of attention_impl.h (see there for the tiling, LDS images and MFMA orientation); this file holds
// their table score source and the host side.  What the source changes is where the score bias comes from and where its
// gradient goes:
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

#include "attention_impl.h"

using namespace htrvt;

namespace {

constexpr float MASKED2 = -1.0e30f;          // score (base-2 domain) of a pair outside the window / a padding key
constexpr int PAD_KEY = 1 << 29, PAD_QUERY = -(1 << 29);

struct RelParams : AttnCore {
  const float* table;  // [2P-1][h] float32
  float* ws_rows;      // backward: [h][B][nqb][2P-1] partial d(table) rows, or NULL (no table gradient)
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

__host__ __device__ inline int tab_floats(int P) { return (2 * P - 1 + 3) / 4 * 4; }

// LDS behind the staged tiles: codes[ncode] | table column | dQ launch: 4 diagonal arrays | 4 [32][33] blocks
struct TableScores {
  using Params = RelParams;
  static constexpr bool GROUPED = false;
  // dQ at hd 128: one workgroup per CU (the diagonal sums need more than the 256 VGPRs of two workgroups per CU: 5 spilled there)
  static constexpr int dq_wgs(int hd) { return hd >= 128 ? 1 : 2; }
  const Params& p;
  const Where& w;
  int* codes;
  float* tabl;
  int crow;                     // code of the lane's own query (forward, dQ) / key (dK/dV)
  int ndiag;                    // dQ, per wave: u = key - query + (wave's first query) + 31
  float *diag_all, *diag, *blk; // dQ: the four diagonal arrays, this wave's, and its [32][33] d(score) block

  __device__ __forceinline__ TableScores(const Params& p, char* lds, const Where& w)
      : p(p), w(w), codes(reinterpret_cast<int*>(lds)), tabl(reinterpret_cast<float*>(codes + p.ncode)) {}

  // windowed attention: a staged tile that none of the workgroup's tokens a0 .. a1 can see is skipped
  __device__ __forceinline__ int first_tile(int len, int a0, int a1) const { return next_live(p, 0, ceil_div(p.N, len), len, a0, a1); }
  __device__ __forceinline__ int next_tile(int t, int len, int a0, int a1) const { return next_live(p, t + 1, ceil_div(p.N, len), len, a0, a1); }
  __device__ __forceinline__ int restage(int t, int tl, int nt) const { return tl < nt ? tl : t; }

  __device__ __forceinline__ void stage() const { stage_codes_table(p, w.hh, codes, tabl); }
  __device__ __forceinline__ void stage_dq() {
    ndiag = ceil_div(p.N, KT) * KT + 32;
    diag_all = tabl + tab_floats(p.P);
    diag = diag_all + w.wave * ndiag;
    blk = diag_all + 4 * ndiag + w.wave * (32 * 33);
    if (p.ws_rows != nullptr)
      for (int u = threadIdx.x; u < 4 * ndiag; u += 256) diag_all[u] = 0.f;
  }
  // padding queries (q > last) get the query sentinel: every pair of theirs is masked, P = 0, d(score) = 0
  __device__ __forceinline__ void bind_query(int q) { crow = q <= w.last ? codes[q] : PAD_QUERY; }
  __device__ __forceinline__ void bind_key(int k) { crow = codes[k]; }       // a padding key's pairs are masked; its row is not stored

  __device__ __forceinline__ float fwd_scores(f32x16_t (&st)[2], int t, int) const {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int4 ck = *reinterpret_cast<const int4*>(codes + t * KT + 32 * c + 8 * g + 4 * w.hf);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float bv = pair_bias(p, tabl, crow, (&ck.x)[j]);
          const float sb = bv == MASKED2 ? MASKED2 : fmaf(st[c][4 * g + j], p.sl2, bv);
          st[c][4 * g + j] = sb;
          mx = fmaxf(mx, sb);
        }
      }
    return fmaxf(mx, xhalf(mx));
  }
  __device__ __forceinline__ float fwd_prob(float s, float mn) const { return fast_exp2(s - mn); }

  __device__ __forceinline__ void dq_scores(f32x16_t& st, f32x16_t& dp, int t, int, int c, float lse, float dl) const {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int4 ck = *reinterpret_cast<const int4*>(codes + t * KT + 32 * c + 8 * g + 4 * w.hf);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bv = pair_bias(p, tabl, crow, (&ck.x)[j]);
        const float pr = bv == MASKED2 ? 0.f : fast_exp2(fmaf(st[4 * g + j], p.sl2, bv - lse));
        st[4 * g + j] = pr * (dp[4 * g + j] - dl);          // d(score) = d(bias entry) of this pair
        dp[4 * g + j] = st[4 * g + j] * p.scale;             // dS
      }
    }
  }
  // d(score) of the 32 x 32 block (t, c) -> the wave's scratch [query r][key kk] (kk = (i & 3) + 8 (i >> 2) + 4 half), then
  // lane L sums diagonal j = kk - r = L - 31 over r = 0 .. 31 in that order (lane 63: none)
  __device__ __forceinline__ void dq_block(const f32x16_t& st, int t, int c) const {
    if (p.ws_rows == nullptr) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) blk[w.r * 33 + (i & 3) + 8 * (i >> 2) + 4 * w.hf] = st[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float acc = 0.f;
#pragma unroll 8
    for (int rr = 0; rr < 32; ++rr) {
      const int kk = rr + w.lane - 31;
      const float v = blk[rr * 33 + min(max(kk, 0), 31)];
      acc += (unsigned)kk < 32u ? v : 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();        // every lane has read the block before the next one is written
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // lane L of this step and lane L - 32 of the next one share a diagonal: volatile keeps the compiler from moving the
    // next step's read (a different address for THIS lane) above this write; the LDS serves one wave in order
    typedef __attribute__((address_space(3))) float lds_float;
    volatile lds_float* du = (volatile lds_float*)(diag + t * KT + 32 * c + w.lane);
    *du = *du + acc;
  }
  // after the key loop: diagonals -> table entries, waves in order; one partial row of 2P-1 floats per workgroup
  __device__ __forceinline__ void dq_end() const {
    if (p.ws_rows == nullptr) return;
    const int ne = 2 * p.P - 1, qa = w.blk * 128;
    float* row = p.ws_rows + ((long long)(w.hh * p.B + w.b) * ((p.N + 127) / 128) + w.blk) * ne;
    for (int e = threadIdx.x; e < ne; e += 256) {
      const int dl0 = e - (p.P - 1);
      // diagonals of entry e: d0 (windowed: only inside the window), and across the cyclic wrap d0 +- Np (shifted windows)
      const bool in0 = p.win <= 0 || (dl0 > -p.win && dl0 < p.win);
      const bool wrap = in0 && p.win > 0 && p.shift > 0;
      float s = 0.f;
      for (int wv = 0; wv < 4; ++wv) {
        const int u = dl0 + qa + 32 * wv + 31;
        if (in0 && u >= 0 && u < ndiag) s += diag_all[wv * ndiag + u];
        if (wrap && u + p.Np >= 0 && u + p.Np < ndiag) s += diag_all[wv * ndiag + u + p.Np];
        if (wrap && u - p.Np >= 0 && u - p.Np < ndiag) s += diag_all[wv * ndiag + u - p.Np];
      }
      row[e] = s;
    }
  }

  // dK/dV: the codes of the quad's four queries
  __device__ __forceinline__ int4 dkv_quad(int q0, int dq) const { return *reinterpret_cast<const int4*>(codes + q0 + dq + 4 * w.hf); }
  __device__ __forceinline__ float dkv_prob(const int4& cq, int j, float s, float ls) const {
    const float bv = pair_bias(p, tabl, (&cq.x)[j], crow);
    return bv == MASKED2 ? 0.f : fast_exp2(fmaf(s, p.sl2, bv - ls));
  }
  __device__ __forceinline__ void dkv_dbias(const int4&, int, float) const {}
};

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

DropParams<RelParams> with_dropout(const RelParams& r, const int64_t* seed, float p) {
  DropParams<RelParams> d{};
  static_cast<RelParams&>(d) = r;
  const DropRate dr = drop_rate(p);
  d.seed = (const long long*)seed;
  d.thr = dr.thr;
  d.keep_scale = dr.scale;
  return d;
}

int fwd_lds(int hd, const RelParams& p) { return 2 * 2 * KT * hd * 2 + 4 * p.ncode + 4 * tab_floats(p.P); }
int dq_lds(int hd, const RelParams& p) { return fwd_lds(hd, p) + 4 * 4 * (ceil_div(p.N, KT) * KT + 32) + 4 * 4 * 32 * 33; }
int dkv_lds(int hd, const RelParams& p) {
  return 2 * (hd == 128 ? DkvGeom<128>::STAGE_B : DkvGeom<64>::STAGE_B) + 4 * p.ncode + 4 * tab_floats(p.P);
}

template <class Drop>
using Launched = typename Drop::template Params<RelParams>;

template <int HD, class Drop>
int launch_fwd(const Launched<Drop>& p, hipStream_t st) {
  constexpr auto kern = attn_fwd_kernel<HD, TableScores, Drop>;
  if (int rc = allow_dynamic_lds<kern>(LDS_MAX, "attn_relpos_fwd")) return rc;
  hipLaunchKernelGGL(kern, dim3(p.B * p.h * ceil_div(p.N, 128)), dim3(256), fwd_lds(HD, p), st, p);
  return check_launch("attn_relpos_fwd");
}

template <int HD, class Drop>
int launch_bwd(const Launched<Drop>& p, float* delta, float* dtable, hipStream_t st) {
  constexpr auto kq = attn_bwd_dq_kernel<HD, TableScores, Drop>;
  constexpr auto kkv = attn_bwd_dkv_kernel<HD, TableScores, Drop>;
  if (int rc = allow_dynamic_lds<kq>(LDS_MAX, "attn_relpos_bwd_dq")) return rc;
  if (int rc = allow_dynamic_lds<kkv>(LDS_MAX, "attn_relpos_bwd_dkv")) return rc;
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

// p == 0: the instantiations without dropout (seed is not read)
template <int HD>
int launch_fwd_p(const RelParams& r, const int64_t* seed, float p, hipStream_t st) {
  if (p == 0.f) return launch_fwd<HD, NoDrop>(r, st);
  return launch_fwd<HD, HashDrop>(with_dropout(r, seed, p), st);
}

template <int HD>
int launch_bwd_p(const RelParams& r, const int64_t* seed, float p, float* delta, float* dtable, hipStream_t st) {
  if (p == 0.f) return launch_bwd<HD, NoDrop>(r, delta, dtable, st);
  return launch_bwd<HD, HashDrop>(with_dropout(r, seed, p), delta, dtable, st);
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
  return htrvt_attn_relpos_dropout_fwd(qkv, table, out, lse2, B, N, heads, hd, scale, num_patches, window, shift, nullptr, 0.f,
                                       dtype, stream);
}

// dropout on the probabilities: p == 0 is the entry point above, seed (an int64 on the device) may then be NULL
extern "C" int htrvt_attn_relpos_dropout_fwd(const void* qkv, const float* table, void* out, float* lse2, int B, int N,
                                             int heads, int hd, float scale, int num_patches, int window, int shift,
                                             const int64_t* seed, float pdrop, int dtype, void* stream) {
  HTRVT_REQUIRE(pdrop >= 0.f && pdrop < 1.f, "htrvt_attn_relpos_fwd: dropout p=%g outside [0, 1)", (double)pdrop);
  HTRVT_REQUIRE(qkv && table && out && (seed || pdrop == 0.f), "htrvt_attn_relpos_fwd: null operand");
  if (int rc = check_geometry(N, hd, dtype, num_patches, window, shift, "htrvt_attn_relpos_fwd")) return rc;
  HTRVT_REQUIRE(B > 0 && heads > 0, "htrvt_attn_relpos_fwd: B=%d heads=%d", B, heads);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_relpos_fwd: qkv too large");
  RelParams p = make_params(qkv, table, B, N, heads, scale, num_patches, window, shift);
  p.out = (bf16_t*)out;
  p.lse2 = lse2;
  HTRVT_REQUIRE(fwd_lds(hd, p) <= LDS_MAX, "htrvt_attn_relpos_fwd: %d B of LDS", fwd_lds(hd, p));
  hipStream_t st = (hipStream_t)stream;
  return hd == 128 ? launch_fwd_p<128>(p, seed, pdrop, st) : launch_fwd_p<64>(p, seed, pdrop, st);
}

extern "C" int htrvt_attn_relpos_bwd(const void* qkv, const float* table, const void* out, const void* dout, const float* lse2,
                                     float* delta, void* dqkv, float* dtable, float* workspace, int B, int N, int heads, int hd,
                                     float scale, int num_patches, int window, int shift, int dtype, void* stream) {
  return htrvt_attn_relpos_dropout_bwd(qkv, table, out, dout, lse2, delta, dqkv, dtable, workspace, B, N, heads, hd, scale,
                                       num_patches, window, shift, nullptr, 0.f, dtype, stream);
}

extern "C" int htrvt_attn_relpos_dropout_bwd(const void* qkv, const float* table, const void* out, const void* dout,
                                             const float* lse2, float* delta, void* dqkv, float* dtable, float* workspace, int B,
                                             int N, int heads, int hd, float scale, int num_patches, int window, int shift,
                                             const int64_t* seed, float pdrop, int dtype, void* stream) {
  HTRVT_REQUIRE(pdrop >= 0.f && pdrop < 1.f, "htrvt_attn_relpos_bwd: dropout p=%g outside [0, 1)", (double)pdrop);
  HTRVT_REQUIRE(qkv && table && out && dout && lse2 && delta && dqkv && (seed || pdrop == 0.f), "htrvt_attn_relpos_bwd: null operand");
  HTRVT_REQUIRE(dtable == nullptr || workspace != nullptr, "htrvt_attn_relpos_bwd: dtable needs the workspace");
  if (int rc = check_geometry(N, hd, dtype, num_patches, window, shift, "htrvt_attn_relpos_bwd")) return rc;
  HTRVT_REQUIRE(B > 0 && heads > 0, "htrvt_attn_relpos_bwd: B=%d heads=%d", B, heads);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_relpos_bwd: qkv too large");
  RelParams p = make_params(qkv, table, B, N, heads, scale, num_patches, window, shift);
  p.out = (bf16_t*)const_cast<void*>(out);
  p.dout = (const bf16_t*)dout;
  p.lse2 = const_cast<float*>(lse2);
  p.dqkv = (bf16_t*)dqkv;
  p.ws_rows = dtable != nullptr ? workspace : nullptr;
  HTRVT_REQUIRE(dq_lds(hd, p) <= LDS_MAX && dkv_lds(hd, p) <= LDS_MAX, "htrvt_attn_relpos_bwd: %d / %d B of LDS",
                dq_lds(hd, p), dkv_lds(hd, p));
  hipStream_t st = (hipStream_t)stream;
  return hd == 128 ? launch_bwd_p<128>(p, seed, pdrop, delta, dtable, st) : launch_bwd_p<64>(p, seed, pdrop, delta, dtable, st);
}
