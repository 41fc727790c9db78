// attention.hip -- fused multi-head self-attention for the HTR-VT encoder block (bfloat16 throughput path, gfx950).
//
// Replaces, per transformer block and direction, the six launches and two [B*h,N,N] HBM round trips of
//   attn = softmax(q @ k^T * scale); x = attn @ v                 (reference model_v1/model/HTR_VT.py:27-36, scale :17)
// and of their autograd backward (train.py:123) by ONE launch each.  The scores S and probabilities P never leave the
// CU: S tiles live in MFMA accumulators, P is rounded to bfloat16 in registers and fed straight back as an MFMA
// operand (accumulator-as-operand k order), K / V (forward) and Q / dO (backward) tiles are staged through LDS.
//
// Layouts (what the qkv Linear writes, HTR_VT.py:29-30): qkv [B*N][3][h][hd] bfloat16, out / dout [B*N][h][hd].
// lse2 [B][h][N] float32 = log2 of the softmax denominator in the scaled base-2 domain:
//   P[q][k] = exp2(S[q][k] * scale * log2(e) - lse2[q]),   saved by the forward for the recomputing backward.
//
// The kernels and their CDNA4 mapping are in attention_impl.h; this file holds the two score sources without a table
// (none / a dense [h][N][N] bias) and the host side.
#include <stdlib.h>

#include "attention_impl.h"

using namespace htrvt;

namespace {

struct AttnParams : AttnCore {
  const float* bias;   // [h][N][N] additive score bias (natural-log units, added after the scale) or NULL
  float* dbias;        // backward: [h][N][N] += sum_b dS (float atomics) or NULL
};

// what a source without LDS state, tile skipping or a bias gradient leaves empty
struct NoExtras : AllTiles {
  using Params = AttnParams;
  static constexpr int dq_wgs(int) { return 2; }
  const Params& p;
  const Where& w;
  __device__ __forceinline__ NoExtras(const Params& p, char*, const Where& w) : p(p), w(w) {}
  __device__ __forceinline__ void stage() const {}
  __device__ __forceinline__ void stage_dq() const {}
  __device__ __forceinline__ void bind_query(int) const {}
  __device__ __forceinline__ void bind_key(int) const {}
  __device__ __forceinline__ void dq_block(const f32x16_t&, int, int) const {}
  __device__ __forceinline__ void dq_end() const {}
  __device__ __forceinline__ int dkv_quad(int, int) const { return 0; }
  __device__ __forceinline__ void dkv_dbias(int, int, float) const {}
};

// no bias: score = S * scale, and -inf on the padding keys of a ragged last tile
struct PlainScores : NoExtras {
  static constexpr bool GROUPED = true;
  using NoExtras::NoExtras;
  __device__ __forceinline__ bool ragged() const { return (p.N % KT) != 0; }       // the last key tile holds padding keys

  // scores of the padding keys of the 32-key block at key0 -> -inf (probability 0)
  __device__ __forceinline__ void mask_padding(f32x16_t& st, int key0) const {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (key0 + (i & 3) + 8 * (i >> 2) + 4 * w.hf > w.last) st[i] = -INFINITY;
  }
  // the scores stay raw: their maximum times sl2 is the maximum score (sl2 > 0), and fwd_prob scales inside its fma
  __device__ __forceinline__ float fwd_scores(f32x16_t (&st)[2], int t, int nt) const {
    if (ragged() && t == nt - 1) {   // workgroup-uniform
#pragma unroll
      for (int c = 0; c < 2; ++c) mask_padding(st[c], t * KT + 32 * c);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, st[c][i]);
    return fmaxf(mx, xhalf(mx)) * p.sl2;
  }
  __device__ __forceinline__ float fwd_prob(float s, float mn) const { return fast_exp2(fmaf(s, p.sl2, -mn)); }
  __device__ __forceinline__ void dq_scores(f32x16_t& st, f32x16_t& dp, int t, int nt, int c, float lse, float dl) const {
    if (ragged() && t == nt - 1) mask_padding(st, t * KT + 32 * c);   // workgroup-uniform
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float pr = fast_exp2(fmaf(st[i], p.sl2, -lse));
      dp[i] = pr * (dp[i] - dl) * p.scale;          // dS^T
    }
  }
  __device__ __forceinline__ float dkv_prob(int, int, float s, float ls) const { return fast_exp2(fmaf(s, p.sl2, -ls)); }
};

// score = S * scale + bias[h][q][k] (relative-position bias, window / padding mask as a large negative number); N is a
// multiple of 128 here, so no tile is ragged
struct DenseScores : NoExtras {
  static constexpr bool GROUPED = false;
  using NoExtras::NoExtras;

  // this lane's query row, four consecutive keys per accumulator register quad
  __device__ __forceinline__ float fwd_scores(f32x16_t (&st)[2], int t, int) const {
    const float* brow = p.bias + ((long long)w.hh * p.N + w.row0 + w.r) * p.N + t * KT + 4 * w.hf;
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 bv = *reinterpret_cast<const float4*>(brow + 32 * c + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          st[c][4 * g + j] = fmaf(st[c][4 * g + j], p.sl2, (&bv.x)[j] * LOG2E);
          mx = fmaxf(mx, st[c][4 * g + j]);
        }
      }
    return fmaxf(mx, xhalf(mx));
  }
  __device__ __forceinline__ float fwd_prob(float s, float mn) const { return fast_exp2(s - mn); }
  __device__ __forceinline__ void dq_scores(f32x16_t& st, f32x16_t& dp, int t, int, int c, float lse, float dl) const {
    const float* brow = p.bias + ((long long)w.hh * p.N + w.row0 + w.r) * p.N + t * KT + 32 * c + 4 * w.hf;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bv = *reinterpret_cast<const float4*>(brow + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float pr = fast_exp2(fmaf(st[4 * g + j], p.sl2, fmaf((&bv.x)[j], LOG2E, -lse)));
        dp[4 * g + j] = pr * (dp[4 * g + j] - dl) * p.scale;
      }
    }
  }
  // dK/dV: bias[h][query][key], the lanes of a half are 32 consecutive keys of one query row.  A quad is the offsets of its
  // four entries, each formed once for the read and the atomic
  struct Quad { long long off[4]; };
  __device__ __forceinline__ Quad dkv_quad(int q0, int dq) const {
    Quad qd;
#pragma unroll
    for (int j = 0; j < 4; ++j) qd.off[j] = ((long long)w.hh * p.N + q0 + dq + 4 * w.hf + j) * p.N + w.row0 + w.r;
    return qd;
  }
  __device__ __forceinline__ float dkv_prob(const Quad& qd, int j, float s, float ls) const {
    return fast_exp2(fmaf(s, p.sl2, fmaf(p.bias[qd.off[j]], LOG2E, -ls)));
  }
  // summed over the batch (skipped when the bias is a constant mask: dbias == NULL)
  __device__ __forceinline__ void dkv_dbias(const Quad& qd, int j, float dsu) const {
    typedef __attribute__((address_space(1))) float gfloat;
    if (p.dbias != nullptr) __hip_atomic_fetch_add((gfloat*)(p.dbias + qd.off[j]), dsu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

template <class Drop>
using Launched = typename Drop::template Params<AttnParams>;

template <int HD, class Src, class Drop>
int launch_fwd(const Launched<Drop>& p, hipStream_t st) {
  constexpr int smem = 2 * 2 * KT * HD * 2;
  if (int rc = allow_dynamic_lds<attn_fwd_kernel<HD, Src, Drop>>(smem, "attn_fwd")) return rc;
  hipLaunchKernelGGL((attn_fwd_kernel<HD, Src, Drop>), dim3(p.B * p.h * ((p.N + 127) / 128)), dim3(256), smem, st, p);
  return check_launch("attn_fwd");
}

template <int HD, class Src, class Drop>
int launch_bwd(const Launched<Drop>& p, float* delta, hipStream_t st) {
  constexpr int smem_dq = 2 * 2 * KT * HD * 2, smem_kv = 2 * DkvGeom<HD>::STAGE_B;
  if (int rc = allow_dynamic_lds<attn_bwd_dq_kernel<HD, Src, Drop>>(smem_dq, "attn_bwd_dq")) return rc;
  if (int rc = allow_dynamic_lds<attn_bwd_dkv_kernel<HD, Src, Drop>>(smem_kv, "attn_bwd_dkv")) return rc;
  const dim3 grid(p.B * p.h * ((p.N + 127) / 128));
  hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, Src, Drop>), grid, dim3(256), smem_dq, st, p, delta);
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<HD, Src, Drop>), grid, dim3(256), smem_kv, st, p, (const float*)delta);
  return check_launch("attn_bwd");
}

template <class Src, class Drop = NoDrop>
int launch(const Launched<Drop>& p, int hd, float* delta, hipStream_t st) {     // delta == NULL: the forward
  if (delta == nullptr)
    return hd == 128 ? launch_fwd<128, Src, Drop>(p, st) : hd == 64 ? launch_fwd<64, Src, Drop>(p, st) : launch_fwd<32, Src, Drop>(p, st);
  return hd == 128 ? launch_bwd<128, Src, Drop>(p, delta, st) : hd == 64 ? launch_bwd<64, Src, Drop>(p, delta, st)
                                                                         : launch_bwd<32, Src, Drop>(p, delta, st);
}

AttnParams make_params(const void* qkv, const float* bias, int B, int N, int heads, float scale) {
  AttnParams p{};
  p.qkv = (const bf16_t*)qkv;
  p.bias = bias;
  p.B = B; p.N = N; p.h = heads;
  p.scale = scale;
  p.sl2 = scale * LOG2E;
  return p;
}

DropParams<AttnParams> with_dropout(const AttnParams& a, const int64_t* seed, float p) {
  DropParams<AttnParams> d{};
  static_cast<AttnParams&>(d) = a;
  const DropRate dr = drop_rate(p);
  d.seed = (const long long*)seed;
  d.thr = dr.thr;
  d.keep_scale = dr.scale;
  return d;
}

}  // namespace

// any sequence length >= 32 (a partial last tile is masked in the kernels); with a score bias: multiples of 128 only
// (the bias rows are read in whole tiles)
extern "C" int htrvt_attn_supported(int N, int hd, int dtype) {
  return dtype == HTRVT_BF16 && N >= 32 && (hd == 32 || hd == 64 || hd == 128);
}

extern "C" int htrvt_attn_fwd(const void* qkv, const float* bias, void* out, float* lse2, int B, int N, int heads, int hd,
                              float scale, int dtype, void* stream) {
  HTRVT_REQUIRE(qkv && out, "htrvt_attn_fwd: null operand");
  HTRVT_REQUIRE(B > 0 && heads > 0 && htrvt_attn_supported(N, hd, dtype),
                "htrvt_attn_fwd: unsupported shape/dtype (N=%d >= 32, hd=%d in {32,64,128}, bfloat16)", N, hd);
  HTRVT_REQUIRE(bias == nullptr || N % 128 == 0, "htrvt_attn_fwd: with a score bias N=%d must be a multiple of 128 (pad, masking the padding keys in the bias)", N);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_fwd: qkv too large");
  AttnParams p = make_params(qkv, bias, B, N, heads, scale);
  p.out = (bf16_t*)out;
  p.lse2 = lse2;
  hipStream_t st = (hipStream_t)stream;
  return bias != nullptr ? launch<DenseScores>(p, hd, nullptr, st) : launch<PlainScores>(p, hd, nullptr, st);
}

extern "C" int htrvt_attn_bwd(const void* qkv, const float* bias, const void* out, const void* dout, const float* lse2,
                              float* delta, void* dqkv, float* dbias, int B, int N, int heads, int hd, float scale, int dtype,
                              void* stream) {
  HTRVT_REQUIRE(qkv && out && dout && lse2 && delta && dqkv, "htrvt_attn_bwd: null operand");
  HTRVT_REQUIRE(B > 0 && heads > 0 && htrvt_attn_supported(N, hd, dtype),
                "htrvt_attn_bwd: unsupported shape/dtype (N=%d >= 32, hd=%d in {32,64,128}, bfloat16)", N, hd);
  HTRVT_REQUIRE(bias == nullptr || N % 128 == 0, "htrvt_attn_bwd: with a score bias N=%d must be a multiple of 128", N);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_bwd: qkv too large");
  HTRVT_REQUIRE(dbias == nullptr || bias != nullptr, "htrvt_attn_bwd: dbias without a bias");   // bias without dbias: a constant mask
  AttnParams p = make_params(qkv, bias, B, N, heads, scale);
  p.out = (bf16_t*)const_cast<void*>(out);
  p.dout = (const bf16_t*)dout;
  p.lse2 = const_cast<float*>(lse2);
  p.dqkv = (bf16_t*)dqkv;
  p.dbias = dbias;
  hipStream_t st = (hipStream_t)stream;
  return bias != nullptr ? launch<DenseScores>(p, hd, delta, st) : launch<PlainScores>(p, hd, delta, st);
}

// ---- dropout on the probabilities (plain scores): the mask of dropout_common.h regenerated in all three kernels ------------
extern "C" int htrvt_attn_dropout_supported(int N, int hd, int dtype) { return htrvt_attn_supported(N, hd, dtype); }

extern "C" int htrvt_attn_dropout_fwd(const void* qkv, void* out, float* lse2, int B, int N, int heads, int hd, float scale,
                                      const int64_t* seed, float p, int dtype, void* stream) {
  HTRVT_REQUIRE(p >= 0.f && p < 1.f, "htrvt_attn_dropout_fwd: p=%g outside [0, 1)", (double)p);
  if (p == 0.f) return htrvt_attn_fwd(qkv, nullptr, out, lse2, B, N, heads, hd, scale, dtype, stream);
  HTRVT_REQUIRE(qkv && out && seed, "htrvt_attn_dropout_fwd: null operand");
  HTRVT_REQUIRE(B > 0 && heads > 0 && htrvt_attn_dropout_supported(N, hd, dtype),
                "htrvt_attn_dropout_fwd: unsupported shape/dtype (N=%d >= 32, hd=%d in {32,64,128}, bfloat16)", N, hd);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_dropout_fwd: qkv too large");
  AttnParams a = make_params(qkv, nullptr, B, N, heads, scale);
  a.out = (bf16_t*)out;
  a.lse2 = lse2;
  return launch<PlainScores, HashDrop>(with_dropout(a, seed, p), hd, nullptr, (hipStream_t)stream);
}

extern "C" int htrvt_attn_dropout_bwd(const void* qkv, const void* out, const void* dout, const float* lse2, float* delta,
                                      void* dqkv, int B, int N, int heads, int hd, float scale, const int64_t* seed, float p,
                                      int dtype, void* stream) {
  HTRVT_REQUIRE(p >= 0.f && p < 1.f, "htrvt_attn_dropout_bwd: p=%g outside [0, 1)", (double)p);
  if (p == 0.f) return htrvt_attn_bwd(qkv, nullptr, out, dout, lse2, delta, dqkv, nullptr, B, N, heads, hd, scale, dtype, stream);
  HTRVT_REQUIRE(qkv && out && dout && lse2 && delta && dqkv && seed, "htrvt_attn_dropout_bwd: null operand");
  HTRVT_REQUIRE(B > 0 && heads > 0 && htrvt_attn_dropout_supported(N, hd, dtype),
                "htrvt_attn_dropout_bwd: unsupported shape/dtype (N=%d >= 32, hd=%d in {32,64,128}, bfloat16)", N, hd);
  HTRVT_REQUIRE((long long)B * N * 3 * heads * hd < (1ll << 31), "htrvt_attn_dropout_bwd: qkv too large");
  AttnParams a = make_params(qkv, nullptr, B, N, heads, scale);
  a.out = (bf16_t*)const_cast<void*>(out);
  a.dout = (const bf16_t*)dout;
  a.lse2 = const_cast<float*>(lse2);
  a.dqkv = (bf16_t*)dqkv;
  return launch<PlainScores, HashDrop>(with_dropout(a, seed, p), hd, delta, (hipStream_t)stream);
}
