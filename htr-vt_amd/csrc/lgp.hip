// lgp.hip -- the three operators the local-global-parallel (LGP) fork adds to the encoder block (model_lgp/model/plg.py),
// around the GEMM / LayerNorm / attention kernels of the hot path:
//   htrvt_attn_local_fwd/bwd     WindowMHSA1D (:109-137) between its qkv and proj Linear layers: self-attention in
//                                non-overlapping windows of w <= 16 tokens.  The reference zero-pads the TOKENS of a ragged last
//                                window in front of the qkv Linear, so a padding slot is a row q = k = v = qkv.bias that real
//                                queries DO attend to; the kernels build those rows from the bias and return their k / v
//                                gradient per image.  Scores never leave the chip and nothing but qkv is saved: the backward
//                                recomputes the (at most 16 x 16) softmax.
//   htrvt_attn_local_shift_*     the same kernels with the Swin-style shift of the SGM local-global fork's WindowMHSA1D
//                                (model_sgm_localglobal/model/HTR_VT.py:118-152: roll, pad, attend, crop, roll back) as
//                                index arithmetic on the token a window slot reads and writes; no mask across the wrap.
//   htrvt_lgp_pool_norm_fwd/bwd  PooledGlobalMHSA (:47-60) up to its qkv Linear: adaptive_avg_pool1d over the tokens fused
//                                with the affine-free LayerNorm of each pooled token.  Backward by gather (a token collects from
//                                the one or two bins that contain it), added onto the gradient that is already there.
//   htrvt_lgp_upsample_fwd/bwd   F.interpolate(mode="linear", align_corners=False) G -> N times sigmoid(logit_alpha) (:69-76),
//                                written with a row stride (the right half of the fuse Linear's [B N][2D] operand).  Backward by
//                                gather, d logit_alpha by a two-stage ordered sum.
// The window attention is the 1-D side of window_attn_impl.h's form: that header's forward kernel over the source below.
// No float atomics anywhere: every result is bitwise reproducible.
#include "window_attn_impl.h"

using namespace htrvt;

namespace {

constexpr int NT = 256;
constexpr int WMAX = 16;          // largest window: one query row per group of four lanes

// ------------------------------------------------------------------ window attention
// The 1-D source of window_attn_impl.h's form: four lanes per row, rows that are no token (the padding slots of a ragged last
// window) built from the qkv bias, nothing added to a score.
struct LocalUnit {
  int b, head, n, nvalid;                  // n = w rows in the window, the first nvalid of them tokens
  long long tok;                           // the token's row of qkv / out
  bool rowact, real;
};

// Shifted windows (WindowMHSA1D with shift s: roll the tokens by s, pad, attend, crop, roll back) are index arithmetic: token j
// sits in rolled slot (j + s) mod N, window t holds slots [t w, t w + w), slots >= N of the last window are the padding rows,
// and slot p < N reads and writes token (p - s) mod N.  `shift` arrives reduced mod N, so that is one compare and one add.
struct Local1d {
  static constexpr int LPR = 4;
  static constexpr bool PADS = true;
  const float* bias;
  int N, heads, w, nW, shift;

  __device__ __forceinline__ LocalUnit unit(long long u, long long units, int r) const {
    LocalUnit x;
    const bool valid = u < units;
    const long long uu = valid ? u : 0;
    x.head = (int)(uu % heads);
    const int win = (int)((uu / heads) % nW);
    x.b = (int)(uu / ((long long)heads * nW));
    const int slot = win * w + r;
    x.tok = (long long)x.b * N + (slot - shift + (slot < shift ? N : 0));
    const int left = N - win * w;          // real slots of this window
    x.n = w;
    x.nvalid = left < w ? left : w;
    x.rowact = valid && r < w;
    x.real = x.rowact && r < x.nvalid;
    return x;
  }
  struct Lds {};
  __device__ __forceinline__ void stage_extras(Lds*, const LocalUnit&, int) const {}
  // padding slot: the k / v row the qkv Linear makes of a zero token
  template <class G>
  __device__ __forceinline__ void pad_row(typename G::Raw* kl, typename G::Raw* vl, const LocalUnit& x, int r, int part) const {
    const int D = heads * G::CPR * G::VN;
    const float* bk = bias + D + x.head * (G::CPR * G::VN);
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      const int c = i * 4 + part;
      typename G::V kk, vv;
#pragma unroll
      for (int e = 0; e < G::VN; ++e) {
        kk.set(e, bk[c * G::VN + e]);
        vv.set(e, bk[D + c * G::VN + e]);
      }
      kl[r * G::RS + c] = kk.raw;
      vl[r * G::RS + c] = vv.raw;
    }
  }
  __device__ __forceinline__ PlainScore score(Lds*, const LocalUnit&) const { return PlainScore{}; }
};

// Backward, one unit per wave and all four matrices (q, k, v, dO) staged at once.  Phase 1, lane (query r, p): P and dS of row
// r (dS times the score scale), left in LDS.  Phase 2: dq[r] = sum_j dS[r][j] k[j]; then, the lane's row taken as key j:
// dk[j] = sum_r dS[r][j] q[r], dv[j] = sum_r P[r][j] dO[r] over the staged q / dO rows.  The `pad` padding keys of a ragged
// window are the same row, so each gets the same gradient: the first of them writes pad x its own into dpad.  (The phases
// are swin.hip's too and stand in both kernels: window_attn_impl.h says why.)
// (3 waves per SIMD asked for as a register cap of 168: the LDS budget limits occupancy to 1 or 2 anyway -- hence the silenced
// "failed to meet occupancy target" --, and left alone the compiler hoists every staged row into registers, takes all 256
// and schedules worse: measured 192 against 130 us.  The pragma spans this one definition; compiled without it the file
// gives exactly three diagnostics, that one for the bf16 hd 128, f32 hd 128 and f32 hd 64 instances -- no failed unroll.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <typename T, int HD, int WPB>
__global__ __launch_bounds__(64 * WPB, 3) void attn_local_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ bias,
                                                                  const T* __restrict__ dout, T* __restrict__ dqkv,
                                                                  float* __restrict__ dpad, int N, int heads, int w, int nW,
                                                                  int shift, float scale, long long units) {
  using G = WinAttnGeom<T, HD, 4>;
  using V = typename G::V;
  using Raw = typename G::Raw;
  __shared__ Raw lds[WPB][4][G::MAT];
  __shared__ float coef[WPB][2][WMAX][WMAX + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane >> 2, p = lane & 3;
  const Local1d win{bias, N, heads, w, nW, shift};
  const LocalUnit x = win.unit((long long)blockIdx.x * WPB + wv, units, r);
  const int D = heads * HD;
  Raw* ql = lds[wv][0];
  Raw* kl = lds[wv][1];
  Raw* vl = lds[wv][2];
  Raw* gl = lds[wv][3];
  float (*Pl)[WMAX + 1] = coef[wv][0];
  float (*Sl)[WMAX + 1] = coef[wv][1];
  Raw q[G::CH], g[G::CH];
#pragma unroll
  for (int i = 0; i < G::CH; ++i) q[i] = g[i] = Raw{};
  if (x.real) {
    const Raw* src = reinterpret_cast<const Raw*>(qkv + x.tok * 3 * D + x.head * HD);
    const Raw* gsrc = reinterpret_cast<const Raw*>(dout + x.tok * D + x.head * HD);
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      const int c = i * 4 + p;
      q[i] = src[c];
      g[i] = gsrc[c];
      ql[r * G::RS + c] = q[i];
      gl[r * G::RS + c] = g[i];
      kl[r * G::RS + c] = src[D / G::VN + c];
      vl[r * G::RS + c] = src[2 * D / G::VN + c];
    }
  } else if (x.rowact) {
    const float* bk = bias + D + x.head * HD;
    V z;
#pragma unroll
    for (int e = 0; e < G::VN; ++e) z.set(e, 0.f);
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      const int c = i * 4 + p;
      V kk, vv;
#pragma unroll
      for (int e = 0; e < G::VN; ++e) {
        kk.set(e, bk[c * G::VN + e]);
        vv.set(e, bk[D + c * G::VN + e]);
      }
      kl[r * G::RS + c] = kk.raw;
      vl[r * G::RS + c] = vv.raw;
      ql[r * G::RS + c] = z.raw;         // a padded query's output is cropped: it sends no gradient
      gl[r * G::RS + c] = z.raw;
    }
  }
  __syncthreads();

  float s[WMAX], dp[WMAX];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < WMAX; ++j) {
    s[j] = -INFINITY;
    dp[j] = 0.f;
    if (j < w) {
      float acc = 0.f, accv = 0.f;
#pragma unroll
      for (int i = 0; i < G::CH; ++i) {
        acc = ChunkDot<T>::run(acc, q[i], kl[j * G::RS + i * 4 + p]);
        accv = ChunkDot<T>::run(accv, g[i], vl[j * G::RS + i * 4 + p]);
      }
      s[j] = row_sum<4>(acc) * scale;
      dp[j] = row_sum<4>(accv);
      m = fmaxf(m, s[j]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < WMAX; ++j)
    if (j < w) {
      s[j] = __expf(s[j] - m);
      sum += s[j];
    }
  const float inv = x.real ? 1.0f / sum : 0.f;   // rows that are no real query: P = dS = 0
  float delta = 0.f;
#pragma unroll
  for (int j = 0; j < WMAX; ++j)
    if (j < w) {
      s[j] *= inv;
      delta += s[j] * dp[j];
    }
  float dq[G::EPL];
#pragma unroll
  for (int e = 0; e < G::EPL; ++e) dq[e] = 0.f;
#pragma unroll
  for (int j = 0; j < WMAX; ++j) {
    if (j < w) {
      dp[j] = s[j] * (dp[j] - delta) * scale;      // dS
      if (p == 0 && r < w) {
        Pl[r][j] = s[j];
        Sl[r][j] = dp[j];
      }
    }
  }
  __syncthreads();

  // dq of this lane's query row.  The coefficients come back from LDS, not from the register arrays above, so that the row
  // loops here need no full unrolling (fully unrolled they took every VGPR and ran slower)
  const int jr = r < w ? r : 0;
#pragma unroll 2
  for (int j = 0; j < w; j += 2) {
    const bool two = j + 1 < w;
    const int j1 = two ? j + 1 : j;
    const auto c = Axpy2<T>::coef(Sl[jr][j], two ? Sl[jr][j1] : 0.f);
#pragma unroll
    for (int i = 0; i < G::CH; ++i)
      Axpy2<T>::run(&dq[i * G::VN], c, kl[j * G::RS + i * 4 + p], kl[j1 * G::RS + i * 4 + p]);
  }
  Raw* drow = reinterpret_cast<Raw*>(dqkv + x.tok * 3 * D + x.head * HD);
  if (x.real) {
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      V a;
#pragma unroll
      for (int e = 0; e < G::VN; ++e) a.set(e, dq[i * G::VN + e]);
      drow[i * 4 + p] = a.raw;
    }
  }

  // phase 2: this lane's row is now key / value row j = r
  float dk[G::EPL], dv[G::EPL];
#pragma unroll
  for (int e = 0; e < G::EPL; ++e) dk[e] = dv[e] = 0.f;
#pragma unroll 2
  for (int i0 = 0; i0 < w; i0 += 2) {          // query rows i0, i1
    const bool two = i0 + 1 < w;
    const int i1 = two ? i0 + 1 : i0;
    const auto cs = Axpy2<T>::coef(Sl[i0][jr], two ? Sl[i1][jr] : 0.f);
    const auto cp = Axpy2<T>::coef(Pl[i0][jr], two ? Pl[i1][jr] : 0.f);
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      Axpy2<T>::run(&dk[i * G::VN], cs, ql[i0 * G::RS + i * 4 + p], ql[i1 * G::RS + i * 4 + p]);
      Axpy2<T>::run(&dv[i * G::VN], cp, gl[i0 * G::RS + i * 4 + p], gl[i1 * G::RS + i * 4 + p]);
    }
  }
  if (x.real) {
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      V a, d;
#pragma unroll
      for (int e = 0; e < G::VN; ++e) {
        a.set(e, dk[i * G::VN + e]);
        d.set(e, dv[i * G::VN + e]);
      }
      drow[D / G::VN + i * 4 + p] = a.raw;
      drow[2 * D / G::VN + i * 4 + p] = d.raw;
    }
  } else if (x.rowact && r == x.nvalid) {        // first padding key of the image's ragged window
    const float npad = (float)(w - x.nvalid);
    float* dst = dpad + (long long)x.b * 2 * D + x.head * HD;
#pragma unroll
    for (int i = 0; i < G::CH; ++i) {
      const int c = i * 4 + p;
#pragma unroll
      for (int e = 0; e < G::VN; ++e) {
        dst[c * G::VN + e] = npad * dk[i * G::VN + e];
        dst[D + c * G::VN + e] = npad * dv[i * G::VN + e];
      }
    }
  }
}

#pragma clang diagnostic pop

// (dtype, hd) served and the waves per workgroup there: what the staged rows leave of the 64 KB of static LDS
#define ATTN_LOCAL_FWD_WPB(X) X(bf16_t, 128, 4) X(bf16_t, 64, 4) X(float, 128, 2) X(float, 64, 4)
#define ATTN_LOCAL_BWD_WPB(X) X(bf16_t, 128, 2) X(bf16_t, 64, 4) X(float, 128, 1) X(float, 64, 2)

int local_check(const char* who, int B, int N, int heads, int hd, int w, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d (float32 or bfloat16)", who, dtype);
  HTRVT_REQUIRE(hd == 64 || hd == 128, "%s: head dim %d (64 or 128)", who, hd);
  HTRVT_REQUIRE(w >= 1 && w <= WMAX, "%s: window=%d outside 1 ... %d", who, w, WMAX);
  HTRVT_REQUIRE(B >= 0 && N >= 1 && heads >= 1, "%s: B=%d N=%d heads=%d", who, B, N, heads);
  return 0;
}

// ------------------------------------------------------------------ pool + LayerNorm
__device__ __forceinline__ int bin_start(int g, int N, int G) { return (int)((long long)g * N / G); }
__device__ __forceinline__ int bin_end(int g, int N, int G) { return (int)(((long long)(g + 1) * N + G - 1) / G); }

constexpr int POOL_MAXD = 2048;   // floats of LDS per wave

// one wave per pooled row; the lane keeps its own columns of the pooled row in LDS between the three passes
template <typename T>
__global__ __launch_bounds__(NT) void pool_norm_fwd_kernel(const T* __restrict__ x, T* __restrict__ z, float* __restrict__ mean,
                                                           float* __restrict__ rstd, long long rows, int N, int G, int D,
                                                           float eps) {
  using V = Vec16<T>;
  using Raw = decltype(V().raw);
  constexpr int VN = V::N;
  __shared__ float buf[NT / 64][POOL_MAXD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * (NT / 64) + wv;
  if (r >= rows) return;
  const int b = (int)(r / G), g = (int)(r % G);
  const int t0 = bin_start(g, N, G), t1 = bin_end(g, N, G);
  const float invlen = 1.0f / (float)(t1 - t0);
  const int nch = D / VN;
  float* mine = buf[wv];
  float sum = 0.f;
  for (int c = lane; c < nch; c += 64) {
    float acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0.f;
    for (int t = t0; t < t1; ++t) {
      V a;
      a.raw = reinterpret_cast<const Raw*>(x + ((long long)b * N + t) * D)[c];
#pragma unroll
      for (int e = 0; e < VN; ++e) acc[e] += a.get(e);
    }
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      const float v = acc[e] * invlen;
      mine[e * (POOL_MAXD / VN) + c] = v;
      sum += v;
    }
  }
  const float mu = wave_sum(sum) / (float)D;
  float var = 0.f;
  for (int c = lane; c < nch; c += 64)
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      const float d = mine[e * (POOL_MAXD / VN) + c] - mu;
      var += d * d;
    }
  const float rs = rsqrtf(wave_sum(var) / (float)D + eps);
  for (int c = lane; c < nch; c += 64) {
    V o;
#pragma unroll
    for (int e = 0; e < VN; ++e) o.set(e, (mine[e * (POOL_MAXD / VN) + c] - mu) * rs);
    reinterpret_cast<Raw*>(z + r * D)[c] = o.raw;
  }
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

// stats[r] = {mean_c(dz), mean_c(dz * z)} of pooled row r
template <typename T>
__global__ __launch_bounds__(NT) void pool_norm_bwd_stats_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                                 float* __restrict__ stats, long long rows, int D) {
  using V = Vec16<T>;
  using Raw = decltype(V().raw);
  constexpr int VN = V::N;
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < D / VN; c += 64) {
    V a, b;
    a.raw = reinterpret_cast<const Raw*>(dz + r * D)[c];
    b.raw = reinterpret_cast<const Raw*>(z + r * D)[c];
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      s1 += a.get(e);
      s2 += a.get(e) * b.get(e);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    stats[2 * r] = s1 / (float)D;
    stats[2 * r + 1] = s2 / (float)D;
  }
}

// dx[t] (+)= sum over the bins g that contain t of rstd_g (dz_g - m1_g - z_g m2_g) / len_g; one thread per (token, chunk)
template <typename T>
__global__ __launch_bounds__(NT) void pool_norm_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                           const float* __restrict__ rstd, const float* __restrict__ stats,
                                                           T* __restrict__ dx, long long total, int N, int G, int D,
                                                           int accumulate) {
  using V = Vec16<T>;
  using Raw = decltype(V().raw);
  constexpr int VN = V::N;
  const int nch = D / VN;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int c = (int)(i % nch);
    const long long row = i / nch;
    const int b = (int)(row / N), t = (int)(row % N);
    const int g0 = (int)((long long)t * G / N), g1 = (int)(((long long)(t + 1) * G + N - 1) / N) - 1;
    float acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0.f;
    for (int g = g0; g <= g1; ++g) {
      const long long pr = (long long)b * G + g;
      const float k = rstd[pr] / (float)(bin_end(g, N, G) - bin_start(g, N, G));
      const float m1 = stats[2 * pr], m2 = stats[2 * pr + 1];
      V a, zz;
      a.raw = reinterpret_cast<const Raw*>(dz + pr * D)[c];
      zz.raw = reinterpret_cast<const Raw*>(z + pr * D)[c];
#pragma unroll
      for (int e = 0; e < VN; ++e) acc[e] += k * (a.get(e) - m1 - zz.get(e) * m2);
    }
    Raw* dst = reinterpret_cast<Raw*>(dx + row * D) + c;
    V o;
    if (accumulate) {
      V old;
      old.raw = *dst;
#pragma unroll
      for (int e = 0; e < VN; ++e) o.set(e, old.get(e) + acc[e]);
    } else {
#pragma unroll
      for (int e = 0; e < VN; ++e) o.set(e, acc[e]);
    }
    *dst = o.raw;
  }
}

// ------------------------------------------------------------------ linear up-sampling
// the taps of output token t, as ATen's upsample_linear1d (align_corners = False)
__device__ __forceinline__ void lerp_taps(int t, int N, int G, int& i0, int& i1, float& lam) {
  const float ratio = (float)G / (float)N;
  float src = ((float)t + 0.5f) * ratio - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  if (i0 > G - 1) i0 = G - 1;
  i1 = i0 + 1 < G ? i0 + 1 : G - 1;
  lam = src - (float)i0;
}

__device__ __forceinline__ float sigmoidf(float a) { return 1.0f / (1.0f + __expf(-a)); }

template <typename T>
__global__ __launch_bounds__(NT) void upsample_fwd_kernel(const T* __restrict__ y, const float* __restrict__ logit_alpha,
                                                          T* __restrict__ out, long long total, int N, int G, int D,
                                                          long long ldo) {
  using V = Vec16<T>;
  using Raw = decltype(V().raw);
  constexpr int VN = V::N;
  const int nch = D / VN;
  const float sg = sigmoidf(logit_alpha[0]);
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int c = (int)(i % nch);
    const long long row = i / nch;
    const int b = (int)(row / N), t = (int)(row % N);
    int i0, i1;
    float lam;
    lerp_taps(t, N, G, i0, i1, lam);
    V a, bb, o;
    a.raw = reinterpret_cast<const Raw*>(y + ((long long)b * G + i0) * D)[c];
    bb.raw = reinterpret_cast<const Raw*>(y + ((long long)b * G + i1) * D)[c];
#pragma unroll
    for (int e = 0; e < VN; ++e) o.set(e, sg * ((1.0f - lam) * a.get(e) + lam * bb.get(e)));
    reinterpret_cast<Raw*>(out + row * ldo)[c] = o.raw;
  }
}

// one wave per pooled row (b, g): dy[g] = sigma sum_t coef(t, g) dout[t] over the tokens that read g, and the block's share
// of sum(dout * interp) = sum_g y[g] . (dy[g] / sigma) into partial[block]
template <typename T>
__global__ __launch_bounds__(NT) void upsample_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ y,
                                                          const float* __restrict__ logit_alpha, T* __restrict__ dy,
                                                          float* __restrict__ partial, long long rows, int N, int G, int D,
                                                          long long ldd) {
  using V = Vec16<T>;
  using Raw = decltype(V().raw);
  constexpr int VN = V::N;
  __shared__ float red[8];
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const float sg = sigmoidf(logit_alpha[0]);
  float dot = 0.f;
  if (r < rows) {
    const int b = (int)(r / G), g = (int)(r % G);
    int tlo = (int)(((double)g - 0.5) * N / G - 0.5) - 2, thi = (int)(((double)g + 1.5) * N / G - 0.5) + 2;
    tlo = tlo < 0 ? 0 : tlo;
    thi = thi > N - 1 ? N - 1 : thi;
    for (int c = lane; c < D / VN; c += 64) {
      float acc[VN];
#pragma unroll
      for (int e = 0; e < VN; ++e) acc[e] = 0.f;
      for (int t = tlo; t <= thi; ++t) {
        int i0, i1;
        float lam;
        lerp_taps(t, N, G, i0, i1, lam);
        const float k = (i0 == g ? 1.0f - lam : 0.f) + (i1 == g ? lam : 0.f);
        if (k != 0.f) {
          V a;
          a.raw = reinterpret_cast<const Raw*>(dout + ((long long)b * N + t) * ldd)[c];
#pragma unroll
          for (int e = 0; e < VN; ++e) acc[e] += k * a.get(e);
        }
      }
      V yy, o;
      yy.raw = reinterpret_cast<const Raw*>(y + r * D)[c];
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        dot += yy.get(e) * acc[e];
        o.set(e, sg * acc[e]);
      }
      reinterpret_cast<Raw*>(dy + r * D)[c] = o.raw;
    }
  }
  dot = block_sum_256(dot, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = dot;
}

// dlogit_alpha += sigma (1 - sigma) sum(partial), one block, fixed order
__global__ __launch_bounds__(NT) void upsample_dalpha_kernel(const float* __restrict__ partial, int n,
                                                             const float* __restrict__ logit_alpha,
                                                             float* __restrict__ dalpha) {
  __shared__ float red[8];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += NT) s += partial[i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) {
    const float sg = sigmoidf(logit_alpha[0]);
    dalpha[0] += sg * (1.0f - sg) * s;
  }
}

inline int blocks_for(long long n, int cap = 8192) {
  long long g = (n + NT - 1) / NT;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

int lgp_check(const char* who, int B, int N, int G, int D, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d (float32 or bfloat16)", who, dtype);
  HTRVT_REQUIRE(B >= 0 && N >= 1 && G >= 1 && G <= N, "%s: B=%d N=%d G=%d (1 <= G <= N)", who, B, N, G);
  const int vn = dtype == HTRVT_BF16 ? 8 : 4;
  HTRVT_REQUIRE(D >= vn && D % vn == 0, "%s: D=%d not a multiple of %d", who, D, vn);
  return 0;
}

}  // namespace

extern "C" int htrvt_attn_local_supported(int hd, int window, int dtype) {
  return local_check("htrvt_attn_local", 0, 1, 1, hd, window, dtype) == 0 ? 1 : 0;
}

static int shift_check(const char* who, int window, int shift) {
  HTRVT_REQUIRE(shift >= 0 && shift < window, "%s: shift=%d outside 0 ... window - 1 = %d", who, shift, window - 1);
  return 0;
}

extern "C" int htrvt_attn_local_shift_supported(int hd, int window, int shift, int dtype) {
  if (local_check("htrvt_attn_local_shift", 0, 1, 1, hd, window, dtype)) return 0;
  return shift_check("htrvt_attn_local_shift", window, shift) == 0 ? 1 : 0;
}

// the two entry points of each direction share one launch; `shift` is checked by the caller and reduced mod N here
static int local_fwd(const char* who, const void* qkv, const float* qkv_bias, void* out, int B, int N, int heads, int hd,
                     int window, int shift, float scale, int dtype, void* stream) {
  if (local_check(who, B, N, heads, hd, window, dtype)) return -1;
  HTRVT_REQUIRE(qkv && qkv_bias && out, "%s: null buffer", who);
  HTRVT_REQUIRE(!misaligned16(qkv, out), "%s: qkv / out must be 16-byte aligned", who);
  const int nW = (N + window - 1) / window;
  const long long units = (long long)B * nW * heads;
  if (units == 0) return 0;
  HTRVT_REQUIRE(units < (1ll << 31), "%s: too many windows", who);
  hipStream_t st = (hipStream_t)stream;
  const int sh = shift % N;
#define WINDOW_ATTN_LAUNCH(T, HD, WPB)                                                                                    \
  hipLaunchKernelGGL((window_attn_fwd_kernel<T, HD, WPB, Local1d>), dim3((unsigned)((units + WPB - 1) / WPB)), dim3(64 * WPB), 0, \
                     st, Local1d{qkv_bias, N, heads, window, nW, sh}, (const T*)qkv, (T*)out, scale, units)
  ATTN_LOCAL_FWD_WPB(WINDOW_ATTN_ROW)
#undef WINDOW_ATTN_LAUNCH
  return check_launch("attn_local_fwd");
}

static int local_bwd(const char* who, const void* qkv, const float* qkv_bias, const void* dout, void* dqkv, float* dpad, int B,
                     int N, int heads, int hd, int window, int shift, float scale, int dtype, void* stream) {
  if (local_check(who, B, N, heads, hd, window, dtype)) return -1;
  HTRVT_REQUIRE(qkv && qkv_bias && dout && dqkv && dpad, "%s: null buffer", who);
  HTRVT_REQUIRE(!misaligned16(qkv, dout, dqkv), "%s: qkv / dout / dqkv must be 16-byte aligned", who);
  const int nW = (N + window - 1) / window;
  const long long units = (long long)B * nW * heads;
  if (units == 0) return 0;
  HTRVT_REQUIRE(units < (1ll << 31), "%s: too many windows", who);
  hipStream_t st = (hipStream_t)stream;
  if (N % window == 0)      // no padding keys: their gradient is zero
    HTRVT_REQUIRE(hipMemsetAsync(dpad, 0, sizeof(float) * 2 * (size_t)B * heads * hd, st) == hipSuccess,
                  "%s: clearing dpad failed", who);
  const int sh = shift % N;
#define WINDOW_ATTN_LAUNCH(T, HD, WPB)                                                                                    \
  hipLaunchKernelGGL((attn_local_bwd_kernel<T, HD, WPB>), dim3((unsigned)((units + WPB - 1) / WPB)), dim3(64 * WPB), 0, st, \
                     (const T*)qkv, qkv_bias, (const T*)dout, (T*)dqkv, dpad, N, heads, window, nW, sh, scale, units)
  ATTN_LOCAL_BWD_WPB(WINDOW_ATTN_ROW)
#undef WINDOW_ATTN_LAUNCH
  return check_launch("attn_local_bwd");
}

extern "C" int htrvt_attn_local_fwd(const void* qkv, const float* qkv_bias, void* out, int B, int N, int heads, int hd,
                                    int window, float scale, int dtype, void* stream) {
  return local_fwd("htrvt_attn_local_fwd", qkv, qkv_bias, out, B, N, heads, hd, window, 0, scale, dtype, stream);
}

extern "C" int htrvt_attn_local_bwd(const void* qkv, const float* qkv_bias, const void* dout, void* dqkv, float* dpad, int B,
                                    int N, int heads, int hd, int window, float scale, int dtype, void* stream) {
  return local_bwd("htrvt_attn_local_bwd", qkv, qkv_bias, dout, dqkv, dpad, B, N, heads, hd, window, 0, scale, dtype, stream);
}

extern "C" int htrvt_attn_local_shift_fwd(const void* qkv, const float* qkv_bias, void* out, int B, int N, int heads, int hd,
                                          int window, int shift, float scale, int dtype, void* stream) {
  if (local_check("htrvt_attn_local_shift_fwd", B, N, heads, hd, window, dtype)) return -1;
  if (shift_check("htrvt_attn_local_shift_fwd", window, shift)) return -1;
  return local_fwd("htrvt_attn_local_shift_fwd", qkv, qkv_bias, out, B, N, heads, hd, window, shift, scale, dtype, stream);
}

extern "C" int htrvt_attn_local_shift_bwd(const void* qkv, const float* qkv_bias, const void* dout, void* dqkv, float* dpad,
                                          int B, int N, int heads, int hd, int window, int shift, float scale, int dtype,
                                          void* stream) {
  if (local_check("htrvt_attn_local_shift_bwd", B, N, heads, hd, window, dtype)) return -1;
  if (shift_check("htrvt_attn_local_shift_bwd", window, shift)) return -1;
  return local_bwd("htrvt_attn_local_shift_bwd", qkv, qkv_bias, dout, dqkv, dpad, B, N, heads, hd, window, shift, scale, dtype,
                   stream);
}

extern "C" int htrvt_lgp_pool_norm_fwd(const void* x, void* z, float* mean, float* rstd, int B, int N, int G, int D, float eps,
                                       int dtype, void* stream) {
  if (lgp_check("htrvt_lgp_pool_norm_fwd", B, N, G, D, dtype)) return -1;
  HTRVT_REQUIRE(D <= POOL_MAXD, "htrvt_lgp_pool_norm_fwd: D=%d > %d", D, POOL_MAXD);
  const long long rows = (long long)B * G;
  if (rows == 0) return 0;
  HTRVT_REQUIRE(x && z && mean && rstd, "htrvt_lgp_pool_norm_fwd: null buffer");
  HTRVT_REQUIRE(!misaligned16(x, z), "htrvt_lgp_pool_norm_fwd: x / z must be 16-byte aligned");
  const dim3 grid((unsigned)((rows + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(pool_norm_fwd_kernel<bf16_t>, grid, dim3(NT), 0, st, (const bf16_t*)x, (bf16_t*)z, mean, rstd, rows, N, G, D, eps);
  else
    hipLaunchKernelGGL(pool_norm_fwd_kernel<float>, grid, dim3(NT), 0, st, (const float*)x, (float*)z, mean, rstd, rows, N, G, D, eps);
  return check_launch("lgp_pool_norm_fwd");
}

extern "C" int htrvt_lgp_pool_norm_bwd(const void* dz, const void* z, const float* rstd, float* workspace, void* dx, int B,
                                       int N, int G, int D, int accumulate, int dtype, void* stream) {
  if (lgp_check("htrvt_lgp_pool_norm_bwd", B, N, G, D, dtype)) return -1;
  const long long rows = (long long)B * G;
  if (rows == 0) return 0;
  HTRVT_REQUIRE(dz && z && rstd && workspace && dx, "htrvt_lgp_pool_norm_bwd: null buffer");
  HTRVT_REQUIRE(!misaligned16(dz, z, dx), "htrvt_lgp_pool_norm_bwd: dz / z / dx must be 16-byte aligned");
  const dim3 grid((unsigned)((rows + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)B * N * (D / (dtype == HTRVT_BF16 ? 8 : 4));
  if (dtype == HTRVT_BF16) {
    hipLaunchKernelGGL(pool_norm_bwd_stats_kernel<bf16_t>, grid, dim3(NT), 0, st, (const bf16_t*)dz, (const bf16_t*)z, workspace, rows, D);
    hipLaunchKernelGGL(pool_norm_bwd_kernel<bf16_t>, dim3(blocks_for(total)), dim3(NT), 0, st, (const bf16_t*)dz, (const bf16_t*)z,
                       rstd, workspace, (bf16_t*)dx, total, N, G, D, accumulate);
  } else {
    hipLaunchKernelGGL(pool_norm_bwd_stats_kernel<float>, grid, dim3(NT), 0, st, (const float*)dz, (const float*)z, workspace, rows, D);
    hipLaunchKernelGGL(pool_norm_bwd_kernel<float>, dim3(blocks_for(total)), dim3(NT), 0, st, (const float*)dz, (const float*)z,
                       rstd, workspace, (float*)dx, total, N, G, D, accumulate);
  }
  return check_launch("lgp_pool_norm_bwd");
}

extern "C" int htrvt_lgp_upsample_fwd(const void* y, const float* logit_alpha, void* out, int64_t ldo, int B, int N, int G,
                                      int D, int dtype, void* stream) {
  if (lgp_check("htrvt_lgp_upsample_fwd", B, N, G, D, dtype)) return -1;
  const int vn = dtype == HTRVT_BF16 ? 8 : 4;
  HTRVT_REQUIRE(ldo >= D && ldo % vn == 0, "htrvt_lgp_upsample_fwd: ldo=%lld (>= D, a multiple of %d)", (long long)ldo, vn);
  if (B == 0) return 0;
  HTRVT_REQUIRE(y && logit_alpha && out, "htrvt_lgp_upsample_fwd: null buffer");
  HTRVT_REQUIRE(!misaligned16(y, out), "htrvt_lgp_upsample_fwd: y / out must be 16-byte aligned");
  const long long total = (long long)B * N * (D / vn);
  const dim3 grid(blocks_for(total));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(upsample_fwd_kernel<bf16_t>, grid, dim3(NT), 0, st, (const bf16_t*)y, logit_alpha, (bf16_t*)out, total, N, G, D, (long long)ldo);
  else
    hipLaunchKernelGGL(upsample_fwd_kernel<float>, grid, dim3(NT), 0, st, (const float*)y, logit_alpha, (float*)out, total, N, G, D, (long long)ldo);
  return check_launch("lgp_upsample_fwd");
}

extern "C" int64_t htrvt_lgp_upsample_bwd_workspace_floats(int B, int G) { return ((int64_t)B * G + 3) / 4; }

extern "C" int htrvt_lgp_upsample_bwd(const void* dout, int64_t ldd, const void* y, const float* logit_alpha, void* dy,
                                      float* dlogit_alpha, float* workspace, int B, int N, int G, int D, int dtype,
                                      void* stream) {
  if (lgp_check("htrvt_lgp_upsample_bwd", B, N, G, D, dtype)) return -1;
  const int vn = dtype == HTRVT_BF16 ? 8 : 4;
  HTRVT_REQUIRE(ldd >= D && ldd % vn == 0, "htrvt_lgp_upsample_bwd: ldd=%lld (>= D, a multiple of %d)", (long long)ldd, vn);
  const long long rows = (long long)B * G;
  if (rows == 0) return 0;
  HTRVT_REQUIRE(dout && y && logit_alpha && dy && dlogit_alpha && workspace, "htrvt_lgp_upsample_bwd: null buffer");
  HTRVT_REQUIRE(!misaligned16(dout, y, dy), "htrvt_lgp_upsample_bwd: dout / y / dy must be 16-byte aligned");
  const int nblk = (int)((rows + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(upsample_bwd_kernel<bf16_t>, dim3(nblk), dim3(NT), 0, st, (const bf16_t*)dout, (const bf16_t*)y, logit_alpha,
                       (bf16_t*)dy, workspace, rows, N, G, D, (long long)ldd);
  else
    hipLaunchKernelGGL(upsample_bwd_kernel<float>, dim3(nblk), dim3(NT), 0, st, (const float*)dout, (const float*)y, logit_alpha,
                       (float*)dy, workspace, rows, N, G, D, (long long)ldd);
  hipLaunchKernelGGL(upsample_dalpha_kernel, dim3(1), dim3(NT), 0, st, workspace, nblk, logit_alpha, dlogit_alpha);
  return check_launch("lgp_upsample_bwd");
}
