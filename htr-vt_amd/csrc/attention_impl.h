// attention_impl.h -- the three launches of the fused bfloat16 attention (forward, dQ, dK/dV), once.  attention.hip
// (plain and dense-bias scores) and attn_relpos.hip (relative-position table) instantiate them with a score SOURCE.
//
// CDNA4 mapping (forward; the backward kernels follow the same scheme with the roles of rows / lanes swapped):
//   * workgroup = 4 waves = 128 queries of one (batch, head); two workgroups per CU (64 KB LDS, <= 256 VGPRs each).
//   * "swapped" products: S^T = K Q^T and O^T = V^T P^T with v_mfma_f32_32x32x16_bf16, so a lane always owns ONE query
//     (column of the accumulator tile): row max / row sum are 31 in-register ops + one cross-half exchange, the online
//     softmax rescale is a per-lane scalar, and P^T (keys in the accumulator registers) is the B operand of the second
//     product without any lane movement.
//   * K is read by rows (ds_read_b128), V transposed (ds_read_b64_tr_b16); both tiles use one XOR-swizzled image that
//     is conflict-free for both kinds of read (tools/lds_bank_check.py applies the banking rules to it).
//   * K/V tiles (64 keys) are double buffered: global loads for the next tile are issued before the MFMAs of this one
//     and written to LDS after them (one barrier per tile).
//
// The kernels own the workgroup mapping, the Q / dO / delta prologue, the tile staging, every MFMA block, the online
// softmax rescale and the stores.  A score source `Src` owns what differs between the families:
//   Src::Params                 kernel parameters, derived from AttnCore
//   Src::GROUPED                dK/dV: request the lse2 / delta quads and the fragments of up to four k-steps ahead of their
//                               MFMAs (needs registers the sources that carry a bias do not have)
//   Src::dq_wgs(hd)             workgroups per CU the dQ launch is compiled for
//   Src(p, lds, w)              lds: the dynamic LDS behind the staged tiles; w: the lane's place (Where)
//   first_tile / next_tile      the staged tiles (len tokens each) the workgroup visits (a0 .. a1: its own tokens)
//   restage                     the tile loaded during tile t: the next one, or some valid tile when there is none
//   stage / stage_dq            prologue: LDS staging beside the first tile's loads
//   bind_query / bind_key       per-lane state of the lane's own row, after the prologue's barrier
//   fwd_scores, fwd_prob        raw S^T accumulators of a key tile -> base-2 scores (returns the lane's maximum) -> P
//   dq_scores, dq_block, dq_end raw S^T, dP^T of a 32-key block -> dS^T in dp (d(score) in st); bias-gradient hooks
//   dkv_quad, dkv_prob, dkv_dbias  dK/dV launch: what the source keeps per register quad (four queries); P of a pair from its
//                               raw score; the pair's d(score) for the bias gradient
//
// Dropout on the probabilities is a third template parameter, a policy `Drop` (NoDrop by default: every statement it adds
// sits behind `if constexpr (Drop::ON)`, and the kernel parameter is Src::Params itself).  HashDrop regenerates the mask
// of dropout_common.h in all three kernels from the pair's logical coordinates,
//     keep(b, head, q, k) = keep_elem(seed, ((b h + head) N + q) N + k, thr),
// which is what htrvt_sgm_dropout draws on a dense [B h][N][N] tensor.  Forward: the row sum and lse2 use the undropped
// P, the P fed to O^T += V^T P^T is keep ? P : 0 and 1 / (1 - p) goes into the final 1 / l.  Backward: dP <- keep ?
// dP / (1 - p) : 0 in front of the source's d(score) (delta = rowsum(dO * O) already equals sum_k P M / (1 - p) dP), and
// dV accumulates dO^T (P M / (1 - p)).
#pragma once

#include "attention_common.h"
#include "dropout_common.h"

namespace {

struct AttnCore {
  const bf16_t* qkv;   // [B*N][3][h][hd]
  bf16_t* out;         // [B*N][h*hd]: written by the forward, read by the backward
  float* lse2;         // [B*h][N]
  const bf16_t* dout;  // backward: gradient of out
  bf16_t* dqkv;        // backward: gradient of qkv
  int B, N, h;
  float sl2;           // scale * log2(e)
  float scale;
};

// the lane's place: (batch, head), block of 128 queries (forward, dQ) or keys (dK/dV) and its own row of that block
struct Where {
  int b, hh, bh, blk;
  int lane, wave, r, hf;
  int row0;            // first row of the wave
  int last;            // N - 1
};

// workgroup -> (batch * head, block): the blocks of one head share an XCD (K/V, Q/dO in its L2)
__device__ __forceinline__ void place_workgroup(const AttnCore& p, Where& w) {
  const int nblk = (p.N + 127) / 128;
  w.last = p.N - 1;
  const int total = gridDim.x;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  w.bh = id / nblk, w.blk = id - w.bh * nblk;
  w.b = w.bh / p.h, w.hh = w.bh - w.b * p.h;
}

// (row0 is set by the kernel, behind its lane_addr)
__device__ __forceinline__ void place_lane(Where& w) {
  w.lane = threadIdx.x & 63, w.wave = threadIdx.x >> 6;
  w.r = w.lane & 31, w.hf = w.lane >> 5;
}

// dropout policies.  Params<P>: the kernel parameter over the source's P
struct NoDrop {
  static constexpr bool ON = false;
  static constexpr bool grouped(int) { return true; }      // dK/dV: may a GROUPED source keep its grouping?
  template <class P> using Params = P;
};

template <class P>
struct DropParams : P {
  const long long* seed;   // int64 on the device
  unsigned thr;            // drop_rate(p)
  float keep_scale;
};

struct HashDrop {
  static constexpr bool ON = true;
  // dK/dV at hd 128 holds 400 registers grouped; with the 64-bit hash state beside the up-front fragments it spilled 63
  static constexpr bool grouped(int hd) { return hd < 128; }
  template <class P> using Params = DropParams<P>;
  // hash input of the pair (row, 0) of head bh; one column further adds DROP_G, one row further DROP_G * N
  template <class P>
  static __device__ __forceinline__ unsigned long long row_input(const P& p, int bh, int row) {
    return hash_input((unsigned long long)p.seed[0], ((unsigned long long)bh * p.N + row) * p.N);
  }
};

// plain and dense-bias scores visit every staged tile
struct AllTiles {
  __device__ __forceinline__ int first_tile(int, int, int) const { return 0; }
  __device__ __forceinline__ int next_tile(int t, int, int, int) const { return t + 1; }
  __device__ __forceinline__ int restage(int, int tl, int nt) const { return min(tl, nt - 1); }
};

// -------------------------------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------------------------------
template <int HD, class Src, class Drop = NoDrop>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const typename Drop::template Params<typename Src::Params> p) {
  constexpr int NTH = 256, QB = 128;
  constexpr int TILE_B = KT * HD * 2;
  constexpr int NS = HD / 16;       // k-steps of the QK^T product
  constexpr int ND = HD / 32;       // 32-row tiles of O^T
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][K tile | V tile] | the source's
  Where w;
  place_workgroup(p, w);
  const int b = w.b, hh = w.hh, last = w.last;
  const long long ld = 3ll * p.h * HD;
  const bf16_t* qbase = p.qkv + (long long)b * p.N * ld + hh * HD;
  const bf16_t* kbase = qbase + p.h * HD;
  const bf16_t* vbase = kbase + p.h * HD;
  place_lane(w);
  const int r = w.r, hf = w.hf;
  const LaneAddr<HD> la = lane_addr<HD>(w.lane);
  const int q0 = w.row0 = w.blk * 128 + w.wave * 32;
  Src src(p, smem + 4 * TILE_B, w);
  const int qrow = min(q0 + r, last);      // a padding query of the last block re-reads the last token; its row is not stored
  const int qa = w.blk * QB, qz = min(qa + QB - 1, last);      // the workgroup's real queries

  // Q^T as the B operand of S^T = K Q^T: lane (r, hf) holds Q[q0 + r][16 s + 8 hf .. + 7]
  bf16x8_t qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    qf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(qbase + (long long)qrow * ld + 16 * s + 8 * hf));

  int t = src.first_tile(KT, qa, qz);
  TileStage<HD, NTH> sk, sv;
  sk.issue(kbase, ld, t * KT, last);
  sv.issue(vbase, ld, t * KT, last);
  src.stage();
  sk.commit(smem);
  sv.commit(smem + TILE_B);
  __syncthreads();
  src.bind_query(q0 + r);

  f32x16_t o[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float m = -INFINITY, l = 0.f;     // running max (scaled base-2 domain) and this lane half's share of the running sum
  unsigned long long zrow = 0;      // dropout: hash input of (this lane's query, key 4 hf)
  if constexpr (Drop::ON) zrow = Drop::row_input(p, w.bh, q0 + r) + DROP_G * (unsigned long long)(4 * hf);

  const int nt = (p.N + KT - 1) / KT;
  for (int it = 0; t < nt; ++it) {
    const char* kt = smem + (it & 1) * 2 * TILE_B;
    const char* vt = kt + TILE_B;
    char* nxt = smem + ((it + 1) & 1) * 2 * TILE_B;
    // the last iteration re-stages a tile into the idle buffer (nothing reads it): no conditional around the loads, so
    // the staging registers stay registers
    const int tl = src.next_tile(t, KT, qa, qz);
    const int tn = src.restage(t, tl, nt);
    sk.issue(kbase, ld, tn * KT, last);
    sv.issue(vbase, ld, tn * KT, last);
    // S^T tiles: keys 32 c .. 32 c + 31 of this tile x the wave's 32 queries
    f32x16_t st[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int i = 0; i < 16; ++i) st[c][i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s)
        st[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<HD>(kt, la, 32 * c, s), qf[s], st[c], 0, 0, 0);
    }
    // online softmax for query r: this lane holds 32 of the tile's 64 keys, lane ^ 32 the other 32
    const float mx = src.fwd_scores(st, t, nt);
    const float mn = fmaxf(m, mx);
    float rs = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        st[c][i] = src.fwd_prob(st[c][i], mn);
        rs += st[c][i];
      }
    if (__any(mn > m)) {      // wave-uniform: the running maximum of some query moved -> rescale what is accumulated
      const float alpha = fast_exp2(m - mn);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] *= alpha;
    }
    l += rs;
    if constexpr (Drop::ON) {       // behind the row sum: l and lse2 are those of the undropped P
      const unsigned long long zt = zrow + DROP_G * (unsigned long long)(t * KT);
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (!keep_hashed(zt + DROP_G * (unsigned long long)(32 * c + (i & 3) + 8 * (i >> 2)), p.thr)) st[c][i] = 0.f;
    }
    // O^T += V^T P^T
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
  float inv = 1.0f / l;
  if constexpr (Drop::ON) inv *= p.keep_scale;
  if (q0 + r <= last) {
    store_lane_rows<ND>(o, p.out + ((long long)b * p.N + q0 + r) * ((long long)p.h * HD) + hh * HD, hf, inv);
    if (hf == 0 && p.lse2 != nullptr) p.lse2[(long long)w.bh * p.N + q0 + r] = m + log2f(l);
  }
}

// -------------------------------------------------------------------------------------------------------------------
// backward, first launch: dQ (and delta = rowsum(dO * O) for the second launch).  Same orientation as the forward: a
// lane owns one query, K / V tiles stream through LDS, P is recomputed from the saved lse2.
//   S^T = K Q^T ; P^T = exp2(S^T sl2 - lse2[q]) ; dP^T = V dO^T ; dS^T = P^T (dP^T - delta[q]) scale ; dQ^T += K^T dS^T
// -------------------------------------------------------------------------------------------------------------------
template <int HD, class Src, class Drop = NoDrop>
__global__ __launch_bounds__(256, Src::dq_wgs(HD)) void attn_bwd_dq_kernel(const typename Drop::template Params<typename Src::Params> p,
                                                                          float* __restrict__ delta) {
  constexpr int NTH = 256, QB = 128;
  constexpr int TILE_B = KT * HD * 2;
  constexpr int NS = HD / 16, ND = HD / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][K tile | V tile] | the source's
  Where w;
  place_workgroup(p, w);
  const int b = w.b, hh = w.hh, last = w.last;
  const long long ld = 3ll * p.h * HD, ldo = (long long)p.h * HD;
  const bf16_t* qbase = p.qkv + (long long)b * p.N * ld + hh * HD;
  const bf16_t* kbase = qbase + p.h * HD;
  const bf16_t* vbase = kbase + p.h * HD;
  place_lane(w);
  const int r = w.r, hf = w.hf;
  const LaneAddr<HD> la = lane_addr<HD>(w.lane);
  const int q0 = w.row0 = w.blk * 128 + w.wave * 32;
  Src src(p, smem + 4 * TILE_B, w);
  const int qa = w.blk * QB, qz = min(qa + QB - 1, last);

  bf16x8_t qf[NS], dof[NS];
  float dl = 0.f;
  const int qrow = min(q0 + r, last);
  {
    const bf16_t* dorow = p.dout + ((long long)b * p.N + qrow) * ldo + hh * HD;
    const bf16_t* orow = p.out + ((long long)b * p.N + qrow) * ldo + hh * HD;
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
  dl += xhalf(dl);                                    // delta[q] = sum_d dO[q][d] O[q][d]
  const float lse = p.lse2[(long long)w.bh * p.N + qrow];
  if (hf == 0 && q0 + r <= last) delta[(long long)w.bh * p.N + q0 + r] = dl;

  int t = src.first_tile(KT, qa, qz);
  TileStage<HD, NTH> sk, sv;
  sk.issue(kbase, ld, t * KT, last);
  sv.issue(vbase, ld, t * KT, last);
  src.stage();
  src.stage_dq();
  sk.commit(smem);
  sv.commit(smem + TILE_B);
  __syncthreads();
  src.bind_query(q0 + r);

  f32x16_t dq[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;
  unsigned long long zrow = 0;      // dropout: hash input of (this lane's query, key 4 hf)
  if constexpr (Drop::ON) zrow = Drop::row_input(p, w.bh, q0 + r) + DROP_G * (unsigned long long)(4 * hf);

  const int nt = (p.N + KT - 1) / KT;
  for (int it = 0; t < nt; ++it) {
    const char* kt = smem + (it & 1) * 2 * TILE_B;
    const char* vt = kt + TILE_B;
    char* nxt = smem + ((it + 1) & 1) * 2 * TILE_B;
    const int tl = src.next_tile(t, KT, qa, qz);
    const int tn = src.restage(t, tl, nt);
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
      if constexpr (Drop::ON) {     // dP of the dropped pairs is 0, of the kept ones dP / (1 - p)
        const unsigned long long zt = zrow + DROP_G * (unsigned long long)(t * KT + 32 * c);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          dp[i] = keep_hashed(zt + DROP_G * (unsigned long long)((i & 3) + 8 * (i >> 2)), p.thr) ? dp[i] * p.keep_scale : 0.f;
      }
      src.dq_scores(st, dp, t, nt, c, lse, dl);
      src.dq_block(st, t, c);
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
  src.dq_end();
}

// -------------------------------------------------------------------------------------------------------------------
// backward, second launch: dK and dV.  A lane owns one KEY (K / V fragments of the wave's 32 keys stay in registers),
// Q / dO tiles stream through LDS (read by rows for S and dP, transposed for dV^T and dK^T), queries sit in the
// accumulator rows, so the per-query constants lse2 / delta are per-register values read (broadcast) from LDS.
//   S = Q K^T ; P = exp2(S sl2 - lse2[q]) ; dP = dO V^T ; dS = P (dP - delta[q]) scale ; dV^T += dO^T P ; dK^T += Q^T dS
// One wave per SIMD (the two 32 x HD accumulator sets + the K / V fragments need > 256 registers).
// -------------------------------------------------------------------------------------------------------------------
template <int HD>
struct DkvGeom {
  // 128-query tiles at hd < 128 (the forward / dQ kernels stage 64 keys): one workgroup per CU leaves 160 KB of LDS, and at
  // N = 256 the whole pass is two tiles -- the second one in flight under the first one's 128 MFMAs per wave.
  // Measured: 128-query tiles pay at hd 64 (286 vs 328 us), not at hd 128 (254 vs 244)
  static constexpr int QT = HD >= 128 ? 64 : 128;
  static constexpr int TILE_B = QT * HD * 2;
  static constexpr int STAGE_B = 2 * TILE_B + 2 * QT * 4 + 16;     // Q tile | dO tile | lse2[QT] | delta[QT] | dump word
};

template <int HD, class Src, class Drop = NoDrop>
__global__ __launch_bounds__(256, 1) void attn_bwd_dkv_kernel(const typename Drop::template Params<typename Src::Params> p,
                                                              const float* __restrict__ delta) {
  constexpr int NTH = 256, KB = 128, QT = DkvGeom<HD>::QT;
  constexpr int TILE_B = DkvGeom<HD>::TILE_B, STAGE_B = DkvGeom<HD>::STAGE_B;
  constexpr int NS = HD / 16, ND = HD / 32;
  constexpr bool GROUPED = Src::GROUPED && Drop::grouped(HD);
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][Q | dO | lse2 | delta | dump] | the source's
  Where w;
  place_workgroup(p, w);
  const int b = w.b, hh = w.hh, last = w.last;
  const long long ld = 3ll * p.h * HD, ldo = (long long)p.h * HD;
  const bf16_t* qbase = p.qkv + (long long)b * p.N * ld + hh * HD;
  const bf16_t* kbase = qbase + p.h * HD;
  const bf16_t* vbase = kbase + p.h * HD;
  const bf16_t* dobase = p.dout + (long long)b * p.N * ldo + hh * HD;
  const float* lsebase = p.lse2 + (long long)w.bh * p.N;
  const float* delbase = delta + (long long)w.bh * p.N;
  place_lane(w);
  const int r = w.r, hf = w.hf;
  const LaneAddr<HD> la = lane_addr<HD>(w.lane);
  const int k0 = w.row0 = w.blk * 128 + w.wave * 32;
  Src src(p, smem + 2 * STAGE_B, w);
  const int ka = w.blk * KB, kz = min(ka + KB - 1, last);      // the workgroup's real keys

  bf16x8_t kf[NS], vf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    kf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(kbase + (long long)min(k0 + r, last) * ld + 16 * s + 8 * hf));
    vf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(vbase + (long long)min(k0 + r, last) * ld + 16 * s + 8 * hf));
  }

  int t = src.first_tile(QT, ka, kz);
  TileStage<HD, NTH, QT> sq, sd;
  // thread < QT: lse2 of query tid of the staged tile; QT <= thread < 2 QT: delta of query tid - QT (other threads
  // re-read entry 0: no branch around the load)
  const float* cbase = threadIdx.x < QT ? lsebase + threadIdx.x : (threadIdx.x < 2 * QT ? delbase + (threadIdx.x - QT) : lsebase);
  const int cslot = threadIdx.x < 2 * QT ? threadIdx.x : 2 * QT;       // slot 2*QT: a dump word behind the two arrays
  const int cidx = threadIdx.x < QT ? (int)threadIdx.x : (threadIdx.x < 2 * QT ? (int)threadIdx.x - QT : 0);   // query of the tile this thread's constant belongs to
  sq.issue(qbase, ld, t * QT, last);
  sd.issue(dobase, ldo, t * QT, last);
  const bool is_lse = threadIdx.x < QT;
  float sc = cbase[min(t * QT + cidx, last) - cidx];
  if (is_lse && t * QT + cidx > last) sc = INFINITY;       // padding query of a partial tile: exp2(s - inf) = 0, no NaN (s is finite)
  src.stage();
  sq.commit(smem);
  sd.commit(smem + TILE_B);
  reinterpret_cast<float*>(smem + 2 * TILE_B)[cslot] = sc;
  __syncthreads();
  src.bind_key(k0 + r);

  f32x16_t dk[ND], dv[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dk[d][i] = dv[d][i] = 0.f;
  // dropout: hash input of (query 4 hf, this lane's key) and the step of one query (the lanes own keys here)
  unsigned long long zcol = 0, zstep = 0;
  if constexpr (Drop::ON) {
    zstep = DROP_G * (unsigned long long)p.N;
    zcol = Drop::row_input(p, w.bh, 4 * hf) + DROP_G * (unsigned long long)(k0 + r);
  }

  const int nt = (p.N + QT - 1) / QT;
  for (int it = 0; t < nt; ++it) {
    const char* qt = smem + (it & 1) * STAGE_B;
    const char* dot = qt + TILE_B;
    const float* cst = reinterpret_cast<const float*>(qt + 2 * TILE_B);
    char* nxt = smem + ((it + 1) & 1) * STAGE_B;
    const int tl = src.next_tile(t, QT, ka, kz);
    const int tn = src.restage(t, tl, nt);
    sq.issue(qbase, ld, tn * QT, last);
    sd.issue(dobase, ldo, tn * QT, last);
    sc = cbase[min(tn * QT + cidx, last) - cidx];
    if (is_lse && tn * QT + cidx > last) sc = INFINITY;
#pragma unroll
    for (int c = 0; c < QT / 32; ++c) {
      f32x16_t st, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = dp[i] = 0.f;
      // One wave per SIMD: nothing but this wave's own instruction stream covers an LDS read, so (GROUPED) the tile's
      // per-query constants of this 32-query block and the fragments of a whole product are requested first and the MFMAs
      // follow (read -> wait -> MFMA one at a time cost ~150 cycles per MFMA)
      float4 lsq[4], deq[4];
      if constexpr (GROUPED) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          lsq[g] = *reinterpret_cast<const float4*>(cst + 32 * c + 8 * g + 4 * hf);
          deq[g] = *reinterpret_cast<const float4*>(cst + QT + 32 * c + 8 * g + 4 * hf);
        }
      }
      constexpr int NSG = !GROUPED ? 1 : (NS >= 4 ? 4 : NS);      // k-steps whose fragments are requested together
#pragma unroll
      for (int s0 = 0; s0 < NS; s0 += NSG) {
        bf16x8_t fq[NSG], fd[NSG];
#pragma unroll
        for (int s = 0; s < NSG; ++s) {
          fq[s] = row_frag<HD>(qt, la, 32 * c, s0 + s);
          fd[s] = row_frag<HD>(dot, la, 32 * c, s0 + s);
        }
#pragma unroll
        for (int s = 0; s < NSG; ++s) {
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fq[s], kf[s0 + s], st, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fd[s], vf[s0 + s], dp, 0, 0, 0);
        }
      }
      // accumulator register i is query 32 c + (i & 3) + 8 (i >> 2) + 4 hf of the tile
      static_for<0, 4>([&](auto G) {
        constexpr int g = decltype(G)::value;
        const float4 ls = GROUPED ? lsq[g] : *reinterpret_cast<const float4*>(cst + 32 * c + 8 * g + 4 * hf);
        const float4 de = GROUPED ? deq[g] : *reinterpret_cast<const float4*>(cst + QT + 32 * c + 8 * g + 4 * hf);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dev[4] = {de.x, de.y, de.z, de.w};
        const auto quad = src.dkv_quad(t * QT, 32 * c + 8 * g);      // queries (tile's first) + (offset) + 4 hf + 0 .. 3
        static_for<0, 4>([&](auto J) {
          constexpr int j = decltype(J)::value, i = 4 * g + j;
          const float pr = src.dkv_prob(quad, j, st[i], lsv[j]);            // (a padding query carries lse2 = +inf: pr = 0)
          float pv = pr, dpi = dp[i];
          if constexpr (Drop::ON) {
            const bool keep = keep_hashed(zcol + zstep * (unsigned long long)(t * QT + 32 * c + 8 * g + j), p.thr);
            pv = keep ? pr * p.keep_scale : 0.f;
            dpi = keep ? dpi * p.keep_scale : 0.f;
          }
          const float dsu = pr * (dpi - dev[j]);                            // d(score): gradient of the bias entry too
          src.dkv_dbias(quad, j, dsu);
          st[i] = pv;                                                       // P (dropout: P M / (1 - p), what multiplied V)
          dp[i] = dsu * p.scale;                                            // dS
        });
      });
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8_t pb = acc_frag(st, s), dsb = acc_frag(dp, s);
        if constexpr (GROUPED) {       // the transposed fragments of a k-step are read before its MFMAs
          bf16x8_t tv[ND], tk[ND];
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            tv[d] = tr_frag<HD>(dot, la, 32 * c, s, d);
            tk[d] = tr_frag<HD>(qt, la, 32 * c, s, d);
          }
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            dv[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tv[d], pb, dv[d], 0, 0, 0);
            dk[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tk[d], dsb, dk[d], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            dv[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<HD>(dot, la, 32 * c, s, d), pb, dv[d], 0, 0, 0);
            dk[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<HD>(qt, la, 32 * c, s, d), dsb, dk[d], 0, 0, 0);
          }
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

}  // namespace
