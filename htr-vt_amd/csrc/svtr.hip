// svtr.hip -- the local attention of the SVTR fork (model_sgm_mms_svtr/model/svtr.py): MultiHeadSelfAttention with
// local=True, between the qkv and proj Linear layers.
//   htrvt_attn_nbr2d_fwd/bwd   every query (h, w) of an H x W token map attends to the keys of its centred kh x kw box,
//                              |h - h'| <= kh / 2 and |w - w'| <= kw / 2, clipped to the map (the fork adds a -inf mask to dense
//                              N x N scores: keys outside the box, and outside the map, do not exist).  qkv, out and dqkv stay
//                              in plain token order.  The forward leaves the row's log-sum-exp; the backward recomputes the
//                              scores from qkv and lse and saves nothing else.
// Unlike the windows of swin.hip / lgp.hip the keys of two neighbouring queries differ, so a workgroup takes a TH x 16 tile
// of queries of one (image, head) and stages the tile's key / value halo, (TH + kh - 1) x (16 + kw - 1) rows, in LDS once;
// rows of the halo that lie outside the map are staged as zeros and never read from memory.  Two lanes per query as in
// swin.hip (window_attn_impl.h: ChunkDot, Axpy2, the DPP lane sum).  Here every lane pair reads its own row of the halo, so the
// products run at the LDS read rate, not the broadcast rate of the windows, and what a launch can keep resident is set by the
// halo's LDS.  Hence:
//   * rows are staged without padding, at a fixed pitch of 16 + 11 - 1 = 26 rows per halo line whatever the box, so that
//     every key of the box is an immediate offset from the lane's own address;
//   * bank conflicts are avoided by the ORDER in which a lane walks its chunks instead: queries c and c + 4 (hd 32,
//     bfloat16: four 64-byte rows per 256-byte bank row) share banks, so the lane of column c takes its chunks in the order
//     i ^ k, k = (c / rows per bank row) mod chunks per lane.  The lanes of one ds_read_b128 group then touch 16 different
//     16-byte slots (MI355X LDS: four groups of 16 lanes per instruction).  The lane's q / dO rows and its accumulators are
//     held in that same order, so the order costs nothing per key.
// The backward is one kernel in two roles.  The box is symmetric, so the queries that see key j are j's own box: with the
// roles swapped (the tile's rows are keys, the staged halo holds q / dO rows with their lse and delta = dO . out) the same
// walk gives dk and dv.  First launch: dq.  Second launch: dk, dv.  Every sum runs in the box's fixed order in one lane pair:
// no float atomics, the same bits every run.
#include "window_attn_impl.h"

using namespace htrvt;

namespace {

constexpr int KH_MAX = 7, KW_MAX = 11;   // the fork's box
constexpr int TW = 16;                   // columns of a workgroup's query tile; its rows TH are the instance's
constexpr int PITCH = TW + KW_MAX - 1;   // staged rows per line of the halo

struct Nbr2d {
  int H, W, heads, kh, kw, tiles_h, tiles_w, th;
  float scale;
};

// what is fixed by (T, HD, TH): chunks per staged row (no padding), rows of the largest halo, threads, LDS
template <typename T, int HD, int TH_>
struct NbrGeom : WinAttnGeom<T, HD, 2> {
  using Base = WinAttnGeom<T, HD, 2>;
  static constexpr int TH = TH_;
  static constexpr int NT = 2 * TH * TW;
  static constexpr int HR = (TH + KH_MAX - 1) * PITCH;
  static constexpr int RPB = 16 / Base::CPR;                 // staged rows per 256-byte bank row
  static constexpr int lds_bytes(bool keys) { return HR * (2 * Base::CPR * 16 + (keys ? 8 : 0)); }
  static_assert(Base::CPR <= 16 && lds_bytes(true) <= 160 * 1024, "LDS");
};

// what the lane is in workgroup `blockIdx.x`: its image and head, its tile row r / column c, its token (h, w), whether that
// token is in the map, the part [dylo, dyhi) x [dxlo, dxhi) of the box that is, and the box rows [wlo, whi) its wave walks
struct Lane {
  long long b;
  int head, th0, tw0, r, c, p, h, w, dylo, dyhi, dxlo, dxhi, wlo, whi;
  bool act;
  long long tok;
};

template <int TH>
__device__ __forceinline__ Lane lane_of(const Nbr2d& g) {
  Lane x;
  long long blk = blockIdx.x;
  x.tw0 = (int)(blk % g.tiles_w) * TW;
  blk /= g.tiles_w;
  x.th0 = (int)(blk % g.tiles_h) * TH;
  blk /= g.tiles_h;
  x.head = (int)(blk % g.heads);
  x.b = blk / g.heads;
  const int t = threadIdx.x >> 1;
  x.p = threadIdx.x & 1;
  x.r = t / TW;
  x.c = t % TW;
  x.h = x.th0 + x.r;
  x.w = x.tw0 + x.c;
  x.act = x.h < g.H && x.w < g.W;
  const int ch = g.kh / 2, cw = g.kw / 2;
  x.dylo = x.act ? max(0, ch - x.h) : 0;
  x.dyhi = x.act ? min(g.kh, g.H + ch - x.h) : 0;
  x.dxlo = x.act ? max(0, cw - x.w) : 0;
  x.dxhi = x.act ? min(g.kw, g.W + cw - x.w) : 0;
  x.tok = x.act ? (x.b * g.H + x.h) * g.W + x.w : 0;
  // a wave holds two rows of the tile: the box rows that reach the map from either of them, the same in every lane
  const int wh = x.th0 + (int)(threadIdx.x >> 6) * 2;
  x.wlo = __builtin_amdgcn_readfirstlane(max(0, ch - (wh + 1)));
  x.whi = __builtin_amdgcn_readfirstlane(min(g.kh, g.H + ch - wh));
  return x;
}

// the 16-byte chunk of its row that the lane (column c, part p) takes as its i-th
template <class G>
__device__ __forceinline__ int chunk_of(int i, int c, int p) {
  return ((i ^ ((c / G::RPB) & (G::CH - 1))) << 1) + p;
}

// the lane's chunks of the row at `src`, in the lane's order
template <class G>
__device__ __forceinline__ void load_own(typename G::Raw* regs, const typename G::Raw* src, int c, int p) {
#pragma unroll
  for (int i = 0; i < G::CH; ++i) regs[i] = src[chunk_of<G>(i, c, p)];
}

template <class G>
__device__ __forceinline__ void store_own(typename G::Raw* dst, int c, int p, const float* v) {
#pragma unroll
  for (int i = 0; i < G::CH; ++i) {
    typename G::V a;
#pragma unroll
    for (int e = 0; e < G::VN; ++e) a.set(e, v[i * G::VN + e]);
    dst[chunk_of<G>(i, c, p)] = a.raw;
  }
}

// Forward.  Pass 1: the scores of the box, in registers (all 77 slots unrolled under the wave-uniform guard wlo <= dy < whi,
// dx < kw: box rows that lie outside the map for both of the wave's rows are skipped; a key outside the map scores -inf).  Pass 2: exp, sum and P v, two keys at a time.
template <typename T, int HD, int TH>
__global__ __launch_bounds__(2 * TH * TW) void nbr2d_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out,
                                                                float* __restrict__ lse, Nbr2d g) {
  using G = NbrGeom<T, HD, TH>;
  using Raw = typename G::Raw;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Raw* kl = reinterpret_cast<Raw*>(smem);
  Raw* vl = kl + G::HR * G::CPR;
  const Lane x = lane_of<TH>(g);
  const int D = g.heads * HD, p = x.p;

  const int hrows = TH + g.kh - 1, hcols = TW + g.kw - 1;
  for (int n = threadIdx.x >> 1; n < hrows * hcols; n += G::NT / 2) {
    const int hh = n / hcols, ww = n - hh * hcols, row = hh * PITCH + ww;
    const int h = x.th0 - g.kh / 2 + hh, w = x.tw0 - g.kw / 2 + ww;
    Raw a[G::CH], b[G::CH];
#pragma unroll
    for (int i = 0; i < G::CH; ++i) a[i] = b[i] = Raw{};
    if (h >= 0 && h < g.H && w >= 0 && w < g.W) {
      const Raw* src = reinterpret_cast<const Raw*>(qkv + ((x.b * g.H + h) * g.W + w) * 3 * D + x.head * HD);
      load_row<G>(a, src + D / G::VN, p);
      load_row<G>(b, src + 2 * D / G::VN, p);
    }
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      kl[row * G::CPR + i * 2 + p] = a[i];
      vl[row * G::CPR + i * 2 + p] = b[i];
    }
  }
  Raw q[G::CH];
#pragma unroll
  for (int i = 0; i < G::CH; ++i) q[i] = Raw{};
  if (x.act) load_own<G>(q, reinterpret_cast<const Raw*>(qkv + x.tok * 3 * D + x.head * HD), x.c, p);
  __syncthreads();

  // the lane's chunks of the halo row of the box's first key; key (dy, dx) lies (dy PITCH + dx) rows on
  const Raw* kb[G::CH];
#pragma unroll
  for (int i = 0; i < G::CH; ++i) kb[i] = kl + (x.r * PITCH + x.c) * G::CPR + chunk_of<G>(i, x.c, p);
  float s[KH_MAX * KW_MAX];
  float m = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < KH_MAX; ++dy) {
#pragma unroll
    for (int dx = 0; dx < KW_MAX; ++dx) {
      s[dy * KW_MAX + dx] = -INFINITY;
      if (dy >= x.wlo && dy < x.whi && dx < g.kw) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < G::CH; ++i) acc = ChunkDot<T>::run(acc, q[i], kb[i][(dy * PITCH + dx) * G::CPR]);
        const float v = row_sum<2>(acc) * g.scale;
        const bool ok = dy >= x.dylo && dy < x.dyhi && dx >= x.dxlo && dx < x.dxhi;
        s[dy * KW_MAX + dx] = ok ? v : -INFINITY;
        m = fmaxf(m, s[dy * KW_MAX + dx]);
      }
    }
  }
  if (!x.act) m = 0.f;                     // a lane that is no query: every weight 0, nothing stored
  float o[G::EPL];
#pragma unroll
  for (int e = 0; e < G::EPL; ++e) o[e] = 0.f;
  float sum = 0.f;
#pragma unroll
  for (int dy = 0; dy < KH_MAX; ++dy) {
#pragma unroll
    for (int dx = 0; dx < KW_MAX; dx += 2) {
      if (dy >= x.wlo && dy < x.whi && dx < g.kw) {
        const bool two = dx + 1 < g.kw;    // an odd box's last column goes alone (its partner: the same row, weight 0)
        const float p0 = __expf(s[dy * KW_MAX + dx] - m);
        const float p1 = (dx + 1 < KW_MAX && two) ? __expf(s[dy * KW_MAX + (dx + 1 < KW_MAX ? dx + 1 : dx)] - m) : 0.f;
        sum += p0 + p1;
        const auto c = Axpy2<T>::coef(p0, p1);
        const int r0 = (G::HR + dy * PITCH + dx) * G::CPR, r1 = two ? r0 + G::CPR : r0;
#pragma unroll
        for (int i = 0; i < G::CH; ++i) Axpy2<T>::run(&o[i * G::VN], c, kb[i][r0], kb[i][r1]);
      }
    }
  }
  if (x.act) {
    const float inv = 1.0f / sum;
#pragma unroll
    for (int e = 0; e < G::EPL; ++e) o[e] *= inv;
    store_own<G>(reinterpret_cast<Raw*>(out + x.tok * D + x.head * HD), x.c, p, o);
    if (lse && p == 0) lse[(x.b * g.heads + x.head) * g.H * g.W + (long long)x.h * g.W + x.w] = m + logf(sum);
  }
}

// Backward, one role per launch.  The tile's rows are `own`, the halo's rows `far`:
//   KEYS = false   own = (q, dO) with the row's lse and delta, far = (k, v):   dq  = scale sum_far dS k
//   KEYS = true    own = (k, v), far = (q, dO) with each row's lse and delta:  dk  = scale sum_far dS q,  dv = sum_far P dO
// P = exp(scale q.k - lse) and dS = P (dO.v - delta) belong to the (query, key) pair, whichever of the two is `own`.
template <typename T, int HD, int TH, bool KEYS>
__global__ __launch_bounds__(2 * TH * TW) void nbr2d_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ out,
                                                                const T* __restrict__ dout, const float* __restrict__ lse,
                                                                T* __restrict__ dqkv, Nbr2d g) {
  using G = NbrGeom<T, HD, TH>;
  using Raw = typename G::Raw;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Raw* al = reinterpret_cast<Raw*>(smem);  // far rows of q or k
  Raw* bl = al + G::HR * G::CPR;           // far rows of dO or v
  float* lse_f = reinterpret_cast<float*>(bl + G::HR * G::CPR);   // KEYS only: lse and delta of the far rows
  float* del_f = lse_f + G::HR;
  const Lane x = lane_of<TH>(g);
  const int D = g.heads * HD, p = x.p;
  const long long lrow = (x.b * g.heads + x.head) * g.H * g.W;

  const int hrows = TH + g.kh - 1, hcols = TW + g.kw - 1;
  for (int n = threadIdx.x >> 1; n < hrows * hcols; n += G::NT / 2) {
    const int hh = n / hcols, ww = n - hh * hcols, row = hh * PITCH + ww;
    const int h = x.th0 - g.kh / 2 + hh, w = x.tw0 - g.kw / 2 + ww;
    const bool in = h >= 0 && h < g.H && w >= 0 && w < g.W;
    const long long tok = in ? (x.b * g.H + h) * g.W + w : 0;
    Raw a[G::CH], b[G::CH];
#pragma unroll
    for (int i = 0; i < G::CH; ++i) a[i] = b[i] = Raw{};
    float dot = 0.f;
    if (in) {
      const Raw* src = reinterpret_cast<const Raw*>(qkv + tok * 3 * D + x.head * HD);
      if constexpr (KEYS) {
        Raw o[G::CH];
        load_row<G>(a, src, p);
        load_row<G>(b, reinterpret_cast<const Raw*>(dout + tok * D + x.head * HD), p);
        load_row<G>(o, reinterpret_cast<const Raw*>(out + tok * D + x.head * HD), p);
#pragma unroll
        for (int i = 0; i < G::CH; ++i) {
          const Vec16<T> vb{b[i]}, vo{o[i]};
#pragma unroll
          for (int e = 0; e < G::VN; ++e) dot += vb.get(e) * vo.get(e);
        }
      } else {
        load_row<G>(a, src + D / G::VN, p);
        load_row<G>(b, src + 2 * D / G::VN, p);
      }
    }
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      al[row * G::CPR + i * 2 + p] = a[i];
      bl[row * G::CPR + i * 2 + p] = b[i];
    }
    if constexpr (KEYS) {
      dot = row_sum<2>(dot);
      if (p == 0) {
        lse_f[row] = in ? lse[lrow + (long long)h * g.W + w] : 0.f;
        del_f[row] = dot;
      }
    }
  }

  Raw oa[G::CH], ob[G::CH];
#pragma unroll
  for (int i = 0; i < G::CH; ++i) oa[i] = ob[i] = Raw{};
  float lse_o = 0.f, del_o = 0.f;
  if (x.act) {
    const Raw* src = reinterpret_cast<const Raw*>(qkv + x.tok * 3 * D + x.head * HD);
    if constexpr (KEYS) {
      load_own<G>(oa, src + D / G::VN, x.c, p);
      load_own<G>(ob, src + 2 * D / G::VN, x.c, p);
    } else {
      Raw o[G::CH];
      load_own<G>(oa, src, x.c, p);
      load_own<G>(ob, reinterpret_cast<const Raw*>(dout + x.tok * D + x.head * HD), x.c, p);
      load_own<G>(o, reinterpret_cast<const Raw*>(out + x.tok * D + x.head * HD), x.c, p);
#pragma unroll
      for (int i = 0; i < G::CH; ++i) {
        const Vec16<T> vb{ob[i]}, vo{o[i]};
#pragma unroll
        for (int e = 0; e < G::VN; ++e) del_o += vb.get(e) * vo.get(e);
      }
      lse_o = lse[lrow + (long long)x.h * g.W + x.w];
    }
  }
  if constexpr (!KEYS) del_o = row_sum<2>(del_o);
  __syncthreads();

  const int row00 = x.r * PITCH + x.c;
  const Raw* ab[G::CH];
#pragma unroll
  for (int i = 0; i < G::CH; ++i) ab[i] = al + row00 * G::CPR + chunk_of<G>(i, x.c, p);
  float da[G::EPL], db[G::EPL];
#pragma unroll
  for (int e = 0; e < G::EPL; ++e) da[e] = db[e] = 0.f;
  for (int dy = x.wlo; dy < x.whi; ++dy) {
    const bool oky = dy >= x.dylo && dy < x.dyhi;
#pragma unroll
    for (int dx = 0; dx < KW_MAX; dx += 2) {
      if (dx < g.kw) {
        const bool two = dx + 1 < g.kw;
        const int f0 = dy * PITCH + dx, f1 = two ? f0 + 1 : f0;            // far rows, from the box's first
        const int a0 = f0 * G::CPR, a1 = f1 * G::CPR, b0 = a0 + G::HR * G::CPR, b1 = a1 + G::HR * G::CPR;
        float s0 = 0.f, s1 = 0.f, t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int i = 0; i < G::CH; ++i) {
          s0 = ChunkDot<T>::run(s0, oa[i], ab[i][a0]);
          s1 = ChunkDot<T>::run(s1, oa[i], ab[i][a1]);
          t0 = ChunkDot<T>::run(t0, ob[i], ab[i][b0]);
          t1 = ChunkDot<T>::run(t1, ob[i], ab[i][b1]);
        }
        s0 = row_sum<2>(s0) * g.scale;
        s1 = row_sum<2>(s1) * g.scale;
        t0 = row_sum<2>(t0);
        t1 = row_sum<2>(t1);
        const bool ok0 = oky && dx >= x.dxlo && dx < x.dxhi, ok1 = oky && two && dx + 1 >= x.dxlo && dx + 1 < x.dxhi;
        const float l0 = KEYS ? lse_f[row00 + f0] : lse_o, l1 = KEYS ? lse_f[row00 + f1] : lse_o;
        const float e0 = KEYS ? del_f[row00 + f0] : del_o, e1 = KEYS ? del_f[row00 + f1] : del_o;
        const float p0 = ok0 ? __expf(s0 - l0) : 0.f, p1 = ok1 ? __expf(s1 - l1) : 0.f;
        const auto cs = Axpy2<T>::coef(p0 * (t0 - e0) * g.scale, p1 * (t1 - e1) * g.scale);
#pragma unroll
        for (int i = 0; i < G::CH; ++i) Axpy2<T>::run(&da[i * G::VN], cs, ab[i][a0], ab[i][a1]);
        if constexpr (KEYS) {
          const auto cp = Axpy2<T>::coef(p0, p1);
#pragma unroll
          for (int i = 0; i < G::CH; ++i) Axpy2<T>::run(&db[i * G::VN], cp, ab[i][b0], ab[i][b1]);
        }
      }
    }
  }
  if (x.act) {
    Raw* drow = reinterpret_cast<Raw*>(dqkv + x.tok * 3 * D + x.head * HD);
    if constexpr (KEYS) {
      store_own<G>(drow + D / G::VN, x.c, p, da);
      store_own<G>(drow + 2 * D / G::VN, x.c, p, db);
    } else {
      store_own<G>(drow, x.c, p, da);
    }
  }
}

// (dtype, hd, rows TH of the query tile) instances: what the largest halo leaves of the CU's 160 KB of LDS.  bfloat16 hd 32
// has two: TH = 8 (49 KB, three workgroups of four waves per CU) and TH = 4 (33 KB, four of two) for maps whose height
// fills tiles of 4 rows better (the fork's last local map is 4 x 128).  128-byte rows: 67 KB, two of two; float32 hd 64: 133 KB
#define NBR2D_KINDS(X) X(bf16_t, 64, 4) X(bf16_t, 32, 8) X(bf16_t, 32, 4) X(float, 64, 4) X(float, 32, 4)
#define NBR2D_ROW(T, HD, TH) \
  if (dtype == (sizeof(T) == 2 ? HTRVT_BF16 : HTRVT_F32) && hd == HD && g.th == TH) NBR2D_LAUNCH(T, HD, TH);

// rows of the query tile for a map of H rows: 8 where that instance exists and leaves no more idle rows than 4 would
int tile_rows(int hd, int dtype, int H) { return (dtype == HTRVT_BF16 && hd == 32 && (H + 7) / 8 * 8 <= (H + 3) / 4 * 4) ? 8 : 4; }

int kind_check(const char* who, int hd, int kh, int kw, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d (float32 or bfloat16)", who, dtype);
  HTRVT_REQUIRE(hd == 32 || hd == 64, "%s: head dim %d (32 or 64)", who, hd);
  HTRVT_REQUIRE(kh >= 1 && kh <= KH_MAX && kw >= 1 && kw <= KW_MAX && (kh & 1) && (kw & 1),
                "%s: box %d x %d (odd sides, at most %d x %d)", who, kh, kw, KH_MAX, KW_MAX);
  return 0;
}

// the geometry of a launch and its workgroups, or -1.  Offsets into the operands are 64-bit throughout (tokens * 3 * heads * hd
// may pass 2^31 elements); what is bounded is the grid
long long map_check(const char* who, Nbr2d* g, int B, int H, int W, int heads, int hd, int kh, int kw, float scale, int dtype) {
  HTRVT_REQUIRE(B >= 0 && H >= 1 && W >= 1 && heads >= 1, "%s: B=%d H=%d W=%d heads=%d", who, B, H, W, heads);
  const int th = tile_rows(hd, dtype, H);
  *g = Nbr2d{H, W, heads, kh, kw, (H + th - 1) / th, (W + TW - 1) / TW, th, scale};
  const long long blocks = (long long)B * heads * g->tiles_h * g->tiles_w;
  HTRVT_REQUIRE(blocks < (1ll << 31) && (long long)H * W < (1ll << 31), "%s: B=%d heads=%d map %d x %d is more than 2^31 - 1 "
                "workgroups of %d x %d queries", who, B, heads, H, W, th, TW);
  return blocks;
}

}  // namespace

extern "C" int htrvt_attn_nbr2d_supported(int hd, int kh, int kw, int dtype) {
  return kind_check("htrvt_attn_nbr2d", hd, kh, kw, dtype) == 0 ? 1 : 0;
}

extern "C" int htrvt_attn_nbr2d_fwd(const void* qkv, void* out, float* lse, int B, int H, int W, int heads, int hd, int kh,
                                    int kw, float scale, int dtype, void* stream) {
  const char* who = "htrvt_attn_nbr2d_fwd";
  if (kind_check(who, hd, kh, kw, dtype)) return -1;
  Nbr2d g;
  const long long blocks = map_check(who, &g, B, H, W, heads, hd, kh, kw, scale, dtype);
  if (blocks < 0) return -1;
  HTRVT_REQUIRE(qkv && out, "%s: null buffer", who);
  HTRVT_REQUIRE(!misaligned16(qkv, out), "%s: qkv / out must be 16-byte aligned", who);
  if (blocks == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define NBR2D_LAUNCH(T, HD, TH)                                                                               \
  {                                                                                                            \
    using G = NbrGeom<T, HD, TH>;                                                                              \
    constexpr auto kern = nbr2d_fwd_kernel<T, HD, TH>;                                                         \
    if (int rc = allow_dynamic_lds<kern>(G::lds_bytes(false), who)) return rc;                                 \
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(G::NT), G::lds_bytes(false), st, (const T*)qkv, (T*)out, lse, g); \
  }
  NBR2D_KINDS(NBR2D_ROW)
#undef NBR2D_LAUNCH
  return check_launch("attn_nbr2d_fwd");
}

extern "C" int htrvt_attn_nbr2d_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B,
                                    int H, int W, int heads, int hd, int kh, int kw, float scale, int dtype, void* stream) {
  const char* who = "htrvt_attn_nbr2d_bwd";
  if (kind_check(who, hd, kh, kw, dtype)) return -1;
  Nbr2d g;
  const long long blocks = map_check(who, &g, B, H, W, heads, hd, kh, kw, scale, dtype);
  if (blocks < 0) return -1;
  HTRVT_REQUIRE(qkv && out && dout && lse && dqkv, "%s: null buffer", who);
  HTRVT_REQUIRE(!misaligned16(qkv, out, dout, dqkv), "%s: qkv / out / dout / dqkv must be 16-byte aligned", who);
  if (blocks == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define NBR2D_LAUNCH(T, HD, TH)                                                                               \
  {                                                                                                            \
    using G = NbrGeom<T, HD, TH>;                                                                              \
    constexpr auto kq = nbr2d_bwd_kernel<T, HD, TH, false>;                                                    \
    constexpr auto kk = nbr2d_bwd_kernel<T, HD, TH, true>;                                                     \
    if (int rc = allow_dynamic_lds<kq>(G::lds_bytes(false), who)) return rc;                                   \
    if (int rc = allow_dynamic_lds<kk>(G::lds_bytes(true), who)) return rc;                                    \
    hipLaunchKernelGGL(kq, dim3((unsigned)blocks), dim3(G::NT), G::lds_bytes(false), st, (const T*)qkv, (const T*)out, \
                       (const T*)dout, lse, (T*)dqkv, g);                                                      \
    hipLaunchKernelGGL(kk, dim3((unsigned)blocks), dim3(G::NT), G::lds_bytes(true), st, (const T*)qkv, (const T*)out, \
                       (const T*)dout, lse, (T*)dqkv, g);                                                      \
  }
  NBR2D_KINDS(NBR2D_ROW)
#undef NBR2D_LAUNCH
  return check_launch("attn_nbr2d_bwd");
}
