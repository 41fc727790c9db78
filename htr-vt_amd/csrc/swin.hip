// swin.hip -- the attention of the Swin fork (model_sgm_mms_swin/model/HTR_VT.py): WindowAttention2D as SwinBlock2D calls it,
// between the qkv and proj Linear layers.
//   htrvt_attn_win2d_fwd/bwd   self-attention inside 2-D windows of wh x ww <= 32 tokens of an H x W token map, with the
//                              learned relative-position bias table, the 2-D cyclic shift and the fork's additive -100 mask
//                              between the wrapped regions (two regions per shifted axis).  qkv, out and dqkv stay in plain
//                              token order: roll, window partition, window reverse and roll-back are index arithmetic on the
//                              token a window slot reads and writes (include/htrvt.h has the formulas).  Scores never leave
//                              the chip and nothing but qkv is saved: the backward recomputes the (at most 32 x 32) softmax.
//                              The table gradient leaves as partial rows for htrvt_rowsum_f32, one per share of the
//                              (image, window) items, each an ordered sum.
// The scores stay on the VALU, in the form of window_attn_impl.h that lgp.hip's 1-D windows share: a 32-token window of a
// 32-wide head is 2 x 32 x 32 x 32 multiply-adds per product, the launch is bound by HBM traffic and load latency, and an MFMA
// tile would have to get the bias, the mask and the softmax out of the accumulator layout for no gain in the bound.
// This file holds what is the 2-D windows' own: the window source of the header's forward kernel (slot-to-token map, table
// entry and mask added to a score) and the backward kernel with its walk over a share's items and the table-gradient gather.
// No float atomics anywhere: every result is bitwise reproducible.
#include "window_attn_impl.h"

using namespace htrvt;

namespace {

constexpr int NMAX = 32;          // largest window: one query row per pair of lanes
constexpr int TMAX = 128;         // table entries per head: (2wh-1)(2ww-1) <= 105 when wh ww <= 32

struct Win2d {
  int H, W, heads, wh, ww, sh, sw, nWw, nWin;   // nWw windows across, nWin = (H / wh) nWw windows per image
  float scale;
};

// what slot t of (image, window) item `item` is: its row / column in the window, its mask region, the token it reads and writes
struct Slot {
  int r, c, reg;
  long long tok;
};

__device__ __forceinline__ Slot win_slot(const Win2d& g, long long item, int t) {
  Slot x;
  const int win = (int)(item % g.nWin);
  const long long b = item / g.nWin;
  x.r = t / g.ww;
  x.c = t - x.r * g.ww;
  const int hs = (win / g.nWw) * g.wh + x.r, ws = (win % g.nWw) * g.ww + x.c;
  x.reg = ((g.sh > 0 && hs >= g.H - g.sh) ? 1 : 0) | ((g.sw > 0 && ws >= g.W - g.sw) ? 2 : 0);
  int th = hs + g.sh, tw = ws + g.sw;
  th -= th >= g.H ? g.H : 0;
  tw -= tw >= g.W ? g.W : 0;
  x.tok = (b * g.H + th) * g.W + tw;
  return x;
}

// what a query needs to know of key slot u: u's offset into the query's span of the table, and u's mask region
__device__ __forceinline__ int key_code(const Win2d& g, const Slot& x) { return (x.r * (2 * g.ww - 1) + x.c) | (x.reg << 8); }
// table entry of (query x, key with offset 0): the key's offset is subtracted from it
__device__ __forceinline__ int query_base(const Win2d& g, const Slot& x) {
  return (x.r + g.wh - 1) * (2 * g.ww - 1) + x.c + g.ww - 1;
}

// score of (query x, key row j) = scale q.k + the pair's table entry - 100 across mask regions; `tbl` is the head's column of
// the table and `key` the key codes of the window's slots, both in LDS
struct Win2dScore {
  const float* tbl;
  const int* key;
  int base, reg;
  __device__ __forceinline__ float operator()(float qk, int j) const {
    const int kc = key[j];
    return qk + tbl[base - (kc & 255)] + ((kc >> 8) != reg ? -100.0f : 0.f);
  }
};

struct Unit2d : Slot {
  int head, n;
  bool rowact, real;
};

// The 2-D source of the form: two lanes per row, every row of a window a token
struct Win2dSource : Win2d {
  static constexpr int LPR = 2;
  static constexpr bool PADS = false;
  struct Lds {
    float tbl[TMAX];
    int key[NMAX];
  };
  const float* table;

  __device__ __forceinline__ Unit2d unit(long long u, long long units, int t) const {
    const bool valid = u < units;
    const long long uu = valid ? u : 0;
    Unit2d x;
    x.n = wh * ww;
    static_cast<Slot&>(x) = win_slot(*this, uu / heads, t < x.n ? t : 0);
    x.head = (int)(uu % heads);
    x.rowact = x.real = valid && t < x.n;
    return x;
  }
  __device__ __forceinline__ void stage_extras(Lds* ext, const Unit2d& x, int lane) const {
    const int TE = (2 * wh - 1) * (2 * ww - 1);
    for (int e = lane; e < TE; e += 64) ext->tbl[e] = table[(long long)e * heads + x.head];
    if ((lane & 1) == 0 && (lane >> 1) < x.n) ext->key[lane >> 1] = key_code(*this, x);
  }
  __device__ __forceinline__ Win2dScore score(const Lds* ext, const Unit2d& x) const {
    return Win2dScore{ext->tbl, ext->key, query_base(*this, x), x.reg};
  }
};

// Backward.  Workgroup (head, share): its WPB waves walk the (image, window) items of partial row `share`, one item per wave
// and step, every wave the same number of steps.  Per item: phase 1, lane (query t, p): P and dS of row t from the staged k / v
// rows, left in LDS (dS without the score scale, which is the table's gradient).  Then dq[t] = scale sum_j dS[t][j] k[j], and
// the wave's share of the table gradient: lane l gathers entries l and l + 64 from dS in key order.  Phase 2 restages q / dO
// over k / v, and the lane's slot taken as key j: dk[j] = scale sum_r dS[r][j] q[r], dv[j] = sum_r P[r][j] dO[r].  After the
// walk the waves' table sums are added in wave order into the partial row.
// (The rows of phase 2 overwrite those of phase 1 so that a float32 head of 128 fits the 64 KB of static LDS.  As in lgp.hip's
// backward the coefficients come back from LDS and the row loops are not fully unrolled.)
template <typename T, int HD, int WPB>
__global__ __launch_bounds__(64 * WPB) void win2d_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ table,
                                                             const T* __restrict__ dout, T* __restrict__ dqkv,
                                                             float* __restrict__ partial, Win2d g, long long items, int rows) {
  using G = WinAttnGeom<T, HD, 2>;
  using V = typename G::V;
  using Raw = typename G::Raw;
  __shared__ Raw lds[WPB][2][G::MAT];
  __shared__ float coef[WPB][2][NMAX][NMAX + 1];
  __shared__ float tbl[TMAX];
  __shared__ float dtab[WPB][TMAX];
  __shared__ int key[WPB][NMAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int head = blockIdx.x, share = blockIdx.y;
  const int n = g.wh * g.ww, t = lane >> 1, p = lane & 1;
  const int D = g.heads * HD, span = 2 * g.ww - 1, TE = (2 * g.wh - 1) * span;
  Raw* kl = lds[wv][0];
  Raw* vl = lds[wv][1];
  float (*Pl)[NMAX + 1] = coef[wv][0];
  float (*Sl)[NMAX + 1] = coef[wv][1];
  for (int e = threadIdx.x; e < TE; e += 64 * WPB) tbl[e] = table[(long long)e * g.heads + head];
  // the two table entries this lane gathers: entry e collects dS[t][u] with (r_t - r_u, c_t - c_u) = (dr, dc)
  int dr[2], dc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int e = lane + 64 * k;
    dr[k] = e / span - (g.wh - 1);
    dc[k] = e % span - (g.ww - 1);
  }
  float tacc[2] = {0.f, 0.f};
  const long long first = items * share / rows, last = items * (share + 1) / rows;
  const int jr = t < n ? t : 0;

  for (long long it = first; it < last; it += WPB) {
    const long long item = it + wv;
    const bool valid = item < last;
    const Slot x = win_slot(g, valid ? item : first, jr);
    const bool act = valid && t < n;
    if (p == 0 && t < n) key[wv][t] = key_code(g, x);
    Raw q[G::CH], go[G::CH];
#pragma unroll
    for (int i = 0; i < G::CH; ++i) q[i] = go[i] = Raw{};
    if (act) {
      const Raw* src = reinterpret_cast<const Raw*>(qkv + x.tok * 3 * D + head * HD);
      const Raw* gsrc = reinterpret_cast<const Raw*>(dout + x.tok * D + head * HD);
#pragma unroll
      for (int i = 0; i < G::CH; ++i) {
        const int c = i * 2 + p;
        q[i] = src[c];
        go[i] = gsrc[c];
        kl[t * G::RS + c] = src[D / G::VN + c];
        vl[t * G::RS + c] = src[2 * D / G::VN + c];
      }
    } else if (t < n) {                    // a wave past the share's end: rows of zeros, so that nothing below reads stale LDS
#pragma unroll
      for (int i = 0; i < G::CH; ++i) kl[t * G::RS + i * 2 + p] = vl[t * G::RS + i * 2 + p] = Raw{};
    }
    __syncthreads();

    const int base = query_base(g, x);
    float s[NMAX], dp[NMAX];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
      s[j] = -INFINITY;
      dp[j] = 0.f;
      if (j < n) {
        float acc = 0.f, accv = 0.f;
#pragma unroll
        for (int i = 0; i < G::CH; ++i) {
          acc = ChunkDot<T>::run(acc, q[i], kl[j * G::RS + i * 2 + p]);
          accv = ChunkDot<T>::run(accv, go[i], vl[j * G::RS + i * 2 + p]);
        }
        const int kc = key[wv][j];
        s[j] = row_sum<2>(acc) * g.scale + tbl[base - (kc & 255)] + ((kc >> 8) != x.reg ? -100.0f : 0.f);
        dp[j] = row_sum<2>(accv);
        m = fmaxf(m, s[j]);
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j < n) {
        s[j] = __expf(s[j] - m);
        sum += s[j];
      }
    const float inv = act ? 1.0f / sum : 0.f;    // rows that are no query: P = dS = 0
    float delta = 0.f;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j < n) {
        s[j] *= inv;
        delta += s[j] * dp[j];
      }
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j < n && p == 0 && t < n) {
        Pl[t][j] = s[j];
        Sl[t][j] = s[j] * (dp[j] - delta);
      }
    __syncthreads();

    float acc[G::EPL];
#pragma unroll
    for (int e = 0; e < G::EPL; ++e) acc[e] = 0.f;
#pragma unroll 2
    for (int j = 0; j < n; j += 2) {
      const bool two = j + 1 < n;
      const int j1 = two ? j + 1 : j;
      const auto c = Axpy2<T>::coef(Sl[jr][j] * g.scale, two ? Sl[jr][j1] * g.scale : 0.f);
#pragma unroll
      for (int i = 0; i < G::CH; ++i)
        Axpy2<T>::run(&acc[i * G::VN], c, kl[j * G::RS + i * 2 + p], kl[j1 * G::RS + i * 2 + p]);
    }
    Raw* drow = reinterpret_cast<Raw*>(dqkv + x.tok * 3 * D + head * HD);
    if (act) {
#pragma unroll
      for (int i = 0; i < G::CH; ++i) {
        V a;
#pragma unroll
        for (int e = 0; e < G::VN; ++e) a.set(e, acc[i * G::VN + e]);
        drow[i * 2 + p] = a.raw;
      }
    }
    // table gradient: in key order u, the query of entry (dr, dc) is slot (r_u + dr, c_u + dc) where the window has one
    for (int ru = 0, cu = 0, uk = 0; uk < n; ++uk) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int rt = ru + dr[k], ct = cu + dc[k];
        if (rt >= 0 && rt < g.wh && ct >= 0 && ct < g.ww) tacc[k] += Sl[rt * g.ww + ct][uk];
      }
      if (++cu == g.ww) {
        cu = 0;
        ++ru;
      }
    }
    __syncthreads();                       // every lane is done with the k / v rows

    if (t < n) {
#pragma unroll
      for (int i = 0; i < G::CH; ++i) {
        kl[t * G::RS + i * 2 + p] = q[i];
        vl[t * G::RS + i * 2 + p] = go[i];
      }
    }
    __syncthreads();

    // phase 2: this lane's slot is now key / value row jr; kl holds the q rows, vl the dO rows
    float dv[G::EPL];
#pragma unroll
    for (int e = 0; e < G::EPL; ++e) acc[e] = dv[e] = 0.f;
#pragma unroll 2
    for (int r = 0; r < n; r += 2) {
      const bool two = r + 1 < n;
      const int r1 = two ? r + 1 : r;
      const auto cs = Axpy2<T>::coef(Sl[r][jr] * g.scale, two ? Sl[r1][jr] * g.scale : 0.f);
      const auto cp = Axpy2<T>::coef(Pl[r][jr], two ? Pl[r1][jr] : 0.f);
#pragma unroll
      for (int i = 0; i < G::CH; ++i) {
        Axpy2<T>::run(&acc[i * G::VN], cs, kl[r * G::RS + i * 2 + p], kl[r1 * G::RS + i * 2 + p]);
        Axpy2<T>::run(&dv[i * G::VN], cp, vl[r * G::RS + i * 2 + p], vl[r1 * G::RS + i * 2 + p]);
      }
    }
    if (act) {
#pragma unroll
      for (int i = 0; i < G::CH; ++i) {
        V a, d;
#pragma unroll
        for (int e = 0; e < G::VN; ++e) {
          a.set(e, acc[i * G::VN + e]);
          d.set(e, dv[i * G::VN + e]);
        }
        drow[D / G::VN + i * 2 + p] = a.raw;
        drow[2 * D / G::VN + i * 2 + p] = d.raw;
      }
    }
    __syncthreads();                       // before the next item's rows and coefficients overwrite these
  }

  dtab[wv][lane] = tacc[0];
  dtab[wv][lane + 64] = tacc[1];
  __syncthreads();
  for (int e = threadIdx.x; e < TE; e += 64 * WPB) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < WPB; ++w) sum += dtab[w][e];
    partial[((long long)share * TE + e) * g.heads + head] = sum;
  }
}

// (dtype, hd) served and the waves per workgroup there, forward and backward: what the staged rows leave of the 64 KB of
// static LDS
#define WIN2D_WPB(X) X(bf16_t, 128, 2) X(bf16_t, 64, 2) X(bf16_t, 32, 4) X(float, 128, 1) X(float, 64, 2) X(float, 32, 2)

int kind_check(const char* who, int hd, int wh, int ww, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d (float32 or bfloat16)", who, dtype);
  HTRVT_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head dim %d (32, 64 or 128)", who, hd);
  HTRVT_REQUIRE(wh >= 1 && ww >= 1 && wh <= NMAX && ww <= NMAX && wh * ww <= NMAX,
                "%s: window %d x %d outside 1 ... %d tokens", who, wh, ww, NMAX);
  return 0;
}

int map_check(const char* who, int B, int H, int W, int heads, int wh, int ww) {
  HTRVT_REQUIRE(B >= 0 && H >= 1 && W >= 1 && heads >= 1 && heads <= 65535, "%s: B=%d H=%d W=%d heads=%d", who, B, H, W, heads);
  HTRVT_REQUIRE(H % wh == 0 && W % ww == 0, "%s: map %d x %d is not a whole number of %d x %d windows", who, H, W, wh, ww);
  return 0;
}

int shift_check(const char* who, int wh, int ww, int sh, int sw) {
  HTRVT_REQUIRE(sh >= 0 && sh < wh && sw >= 0 && sw < ww, "%s: shift (%d, %d) outside its window %d x %d", who, sh, sw, wh, ww);
  return 0;
}

constexpr int MAX_ROWS = 256;     // partial rows of the table gradient: one workgroup per head and row, at most

inline long long win2d_items(int B, int H, int W, int wh, int ww) { return (long long)B * (H / wh) * (W / ww); }
inline int win2d_rows(long long items) { return (int)(items < MAX_ROWS ? (items < 1 ? 1 : items) : MAX_ROWS); }

inline Win2d win2d_geom(int H, int W, int heads, int wh, int ww, int sh, int sw, float scale) {
  return Win2d{H, W, heads, wh, ww, sh, sw, W / ww, (H / wh) * (W / ww), scale};
}

}  // namespace

extern "C" int htrvt_attn_win2d_supported(int hd, int wh, int ww, int dtype) {
  return kind_check("htrvt_attn_win2d", hd, wh, ww, dtype) == 0 ? 1 : 0;
}

extern "C" int htrvt_attn_win2d_rows(int B, int H, int W, int heads, int wh, int ww) {
  HTRVT_REQUIRE(wh >= 1 && ww >= 1, "htrvt_attn_win2d_rows: window %d x %d", wh, ww);
  if (map_check("htrvt_attn_win2d_rows", B, H, W, heads, wh, ww)) return -1;
  return win2d_rows(win2d_items(B, H, W, wh, ww));
}

extern "C" int htrvt_attn_win2d_fwd(const void* qkv, const float* table, void* out, int B, int H, int W, int heads, int hd,
                                    int wh, int ww, int sh, int sw, float scale, int dtype, void* stream) {
  const char* who = "htrvt_attn_win2d_fwd";
  if (kind_check(who, hd, wh, ww, dtype) || map_check(who, B, H, W, heads, wh, ww) || shift_check(who, wh, ww, sh, sw)) return -1;
  HTRVT_REQUIRE(qkv && table && out, "%s: null buffer", who);
  HTRVT_REQUIRE(!misaligned16(qkv, out), "%s: qkv / out must be 16-byte aligned", who);
  const long long units = win2d_items(B, H, W, wh, ww) * heads;
  if (units == 0) return 0;
  HTRVT_REQUIRE(units < (1ll << 31), "%s: too many windows", who);
  const Win2d g = win2d_geom(H, W, heads, wh, ww, sh, sw, scale);
  hipStream_t st = (hipStream_t)stream;
#define WINDOW_ATTN_LAUNCH(T, HD, WPB)                                                                              \
  hipLaunchKernelGGL((window_attn_fwd_kernel<T, HD, WPB, Win2dSource>), dim3((unsigned)((units + WPB - 1) / WPB)), \
                     dim3(64 * WPB), 0, st, Win2dSource{g, table}, (const T*)qkv, (T*)out, scale, units)
  WIN2D_WPB(WINDOW_ATTN_ROW)
#undef WINDOW_ATTN_LAUNCH
  return check_launch("attn_win2d_fwd");
}

extern "C" int htrvt_attn_win2d_bwd(const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable_partial,
                                    int B, int H, int W, int heads, int hd, int wh, int ww, int sh, int sw, float scale,
                                    int dtype, void* stream) {
  const char* who = "htrvt_attn_win2d_bwd";
  if (kind_check(who, hd, wh, ww, dtype) || map_check(who, B, H, W, heads, wh, ww) || shift_check(who, wh, ww, sh, sw)) return -1;
  HTRVT_REQUIRE(qkv && table && dout && dqkv && dtable_partial, "%s: null buffer", who);
  HTRVT_REQUIRE(!misaligned16(qkv, dout, dqkv), "%s: qkv / dout / dqkv must be 16-byte aligned", who);
  const long long items = win2d_items(B, H, W, wh, ww);
  const int rows = win2d_rows(items);
  hipStream_t st = (hipStream_t)stream;
  if (items == 0) {                        // the one partial row of an empty batch
    HTRVT_REQUIRE(hipMemsetAsync(dtable_partial, 0, sizeof(float) * (2 * wh - 1) * (2 * ww - 1) * (size_t)heads, st) == hipSuccess,
                  "%s: clearing dtable_partial failed", who);
    return 0;
  }
  HTRVT_REQUIRE(items * heads < (1ll << 31), "%s: too many windows", who);
  const Win2d g = win2d_geom(H, W, heads, wh, ww, sh, sw, scale);
#define WINDOW_ATTN_LAUNCH(T, HD, WPB)                                                                             \
  hipLaunchKernelGGL((win2d_bwd_kernel<T, HD, WPB>), dim3(heads, rows), dim3(64 * WPB), 0, st, (const T*)qkv, table, \
                     (const T*)dout, (T*)dqkv, dtable_partial, g, items, rows)
  WIN2D_WPB(WINDOW_ATTN_ROW)
#undef WINDOW_ATTN_LAUNCH
  return check_launch("attn_win2d_bwd");
}
